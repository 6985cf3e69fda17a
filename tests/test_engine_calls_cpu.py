"""What HipEngine hands to the C ABI, held on the CPU: the Python counterpart of tests/test_enqueue_table_cpu.py.  Every public method
runs on CPU tensors against a stand-in library (tests/helpers/engine_standin.py) that answers every name of _lib.SIGNATURES, asserts the
argument count and puts each argument through its argtype's from_param.  tests/helpers/engine_cases.py holds the calls: each method
accepted with every optional operand present and absent, and every raise of the host side reached with exactly one thing wrong.  A
section is one call: a line per C entry (integers and floats by value, pointers by the operand, result, workspace or uploaded table they
point at, as base + byte offset), a line per uploaded table by value, then the dtypes and shapes returned or the exception's type and
full text.  The lines must equal tests/golden/engine_calls.txt.gz, recorded at the commit its first line names."""
import gzip

from tests.helpers.engine_cases import GOLDEN, run
from tests.helpers.engine_standin import QUERIES


def test_every_engine_method_makes_the_recorded_calls():
    got, sections = run()
    with gzip.open(GOLDEN, "rt") as f:
        head, *want = f.read().splitlines()
    assert head.startswith("# recorded at ")
    assert len(want) > 1000
    body = {t: sec[1:] for t, (sec, lib) in sections.items()}
    # the table itself holds what the calls were chosen for
    refused = [(t, lib) for t, (sec, lib) in sections.items() if t.startswith("refused: ")]
    assert len(refused) > 120 and all(lib.error is not None for t, lib in refused)
    assert all(lib.error is None for t, (sec, lib) in sections.items() if not t.startswith("refused: "))
    for t, lib in refused:     # a refused call asks for sizes at the most (what the library itself turns down has of course been made)
        made = [name for name, args in lib.calls if not (name.endswith("_bytes") or name in QUERIES)]
        assert not made or made[-1] in lib.fail, (t, made)
    heads = {}
    for t, entry in (("sample plain", "smtts_sample"), ("sample align", "smtts_sample_align"), ("sample pinned", "smtts_sample_pinned"),
                     ("sample pinned align", "smtts_sample_pinned")):
        name, *args = body[t][1].split(" ")
        assert name == entry and body[t][0].startswith("smtts_sample_workspace_bytes ")
        heads[t] = [a.replace("ret[0]", "ret") for a in args[:24]]      # x is the only result of the plain call, else the first
    assert len(heads["sample plain"]) == 24 and all(h == heads["sample plain"] for h in heads.values())
    assert body["deliver pooled 16 kHz"][2] == "table0 int64(2, 4) [[2, 7, 40, 0], [0, 9, 24, 1]]"       # (slot, n_before, len, last)
    assert body["deliver pooled 16 kHz mark mark_state"][-2] == "table0 int64(2, 4) [[2, 7, 40, 0], [0, 9, 24, 0]]"
    assert body["watermark state"][-2] == "table0 int64(2, 4) [[2, 7, 40, 0], [0, 9, 24, 0]]"
    assert sum(l.startswith("smtts_") for l in body["deliver pooled 16 kHz mark mark_state"]) == 4      # two size queries, mark, deliver
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff, f"{len(diff)} lines differ, first: {diff[0]}"
    assert len(got) == len(want)
