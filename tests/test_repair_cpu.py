"""CPU: repair (re-speak only the badly aligned words of a take): the numpy restatement of the two kernels on planted
text-mass buffers, the keep rule, the settings object, the seeds and the command line.  The GPU half (tests/test_repair_gpu.py) holds
the kernels to this restatement exactly."""
import json
import re

import numpy as np
import pytest

from smalltts_amd import _lib, api
from tests.helpers import repair_ref as R
from tests.helpers import takes_ref as T
from tests.helpers.align_ref import dp_align

F32, I32 = np.float32, np.int32


def plan(m, N, P, p0, **kw):
    spans, _score, _path = dp_align(m, N, p0, P)
    pin, counts = R.repair_plan_ref(m[None], spans[None], [N], [p0], [P], **kw)
    return pin[0], tuple(int(v) for v in counts[0])


def freed(pin):
    return np.flatnonzero(pin == 0).tolist()


# (bad tokens, freed frames) at tau 0.1, max_span 8, margin 2; None: not checked
PLANS = {(40, 15, 0): dict(clean=(0, 0), skip=(1, 5), stall=(1, 23), idle=(2, 6)),
         (33, 15, 3): dict(clean=(0, 0), skip=(1, 5), stall=(1, 19), idle=(2, 6)),
         (12, 5, 0): dict(clean=(0, 0), skip=(1, 5), stall=(0, 0), idle=None),
         (225, 198, 0): dict(clean=(0, 0), skip=(1, 5), stall=(1, 23), idle=None)}
FREED = {((40, 15, 0), "skip"): list(range(4, 9)), ((40, 15, 0), "stall"): list(range(9, 32)), ((12, 5, 0), "skip"): list(range(3, 8))}


@pytest.mark.parametrize("shape", T.SHAPES)
def test_the_plan_frees_what_was_planted(shape):
    N, P, p0 = shape
    for v in T.VARIANTS:
        want = PLANS[shape][v]
        if want is None:
            continue
        pin, counts = plan(T.planted(N, P, p0, v), N, P, p0)
        assert counts == want, (shape, v, counts)
        assert int((pin == 0).sum()) == counts[1] and pin.dtype == np.uint8
        if (shape, v) in FREED:
            assert freed(pin) == FREED[(shape, v)], (shape, v, freed(pin))
    if shape == (12, 5, 0):                                      # the stall that is not one: every span at most 8 frames
        spans = dp_align(T.planted(N, P, p0, "stall"), N, p0, P)[0]
        assert int((spans[:, 1] - spans[:, 0] + 1).max()) <= 8


def test_margin_clamps_at_both_ends_and_keep_overrides():
    N, P = 10, 3
    m = np.full((N, P), F32(0.5), F32)
    m[:, 0] = m[:, 2] = F32(0.0)                                 # tokens 0 and 2 are never attended to
    spans = np.asarray([[0, 1], [2, 7], [8, 9]], I32)
    for margin, want in ((0, [0, 1, 8, 9]), (1, [0, 1, 2, 7, 8, 9]), (3, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]), (32, list(range(10)))):
        pin, counts = R.repair_plan_ref(m[None], spans[None], [N], [0], [P], margin=margin)
        assert freed(pin[0]) == want and counts[0].tolist() == [2, len(want)], margin
    # n < N: nothing behind the row's frames is pinned or freed, and the clamp is to n - 1
    pin, counts = R.repair_plan_ref(m[None], spans[None], [9], [0], [P], margin=0)
    assert pin[0].tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0] and counts[0].tolist() == [2, 3]
    # keep overrides a freed frame and is not counted as free; a keep behind n pins nothing
    keep = np.zeros((1, N), bool)
    keep[0, [1, 5, 9]] = True
    pin, counts = R.repair_plan_ref(m[None], spans[None], [9], [0], [P], keep=keep, margin=0)
    assert pin[0].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 0, 0] and counts[0].tolist() == [2, 2]
    # max_span: the middle token is attended to but six frames long
    pin, counts = R.repair_plan_ref(m[None], spans[None], [N], [0], [P], max_span=5, margin=0)
    assert counts[0].tolist() == [3, 10]
    pin, counts = R.repair_plan_ref(m[None], spans[None], [N], [0], [P], max_span=6, margin=0)
    assert counts[0].tolist() == [2, 4]


def test_a_value_at_the_threshold_attends_and_a_nan_does_not():
    N, P = 4, 3
    tau = F32(0.1)
    m = np.full((N, P), np.nextafter(tau, F32(0)), F32)
    spans = np.asarray([[0, 0], [1, 2], [3, 3]], I32)
    args = (spans[None], [N], [0], [P])
    pin, counts = R.repair_plan_ref(m[None], *args, margin=0)
    assert counts[0].tolist() == [3, 4] and not pin.any()
    m2 = m.copy()
    m2[0, 0] = m2[2, 1] = m2[3, 2] = tau                        # exactly at it: attended
    pin, counts = R.repair_plan_ref(m2[None], *args, margin=0)
    assert counts[0].tolist() == [0, 0] and pin.all()
    m3 = m2.copy()
    m3[0, 0] = np.nan                                           # a NaN satisfies no comparison
    pin, counts = R.repair_plan_ref(m3[None], *args, margin=0)
    assert counts[0].tolist() == [1, 1] and pin[0].tolist() == [0, 1, 1, 1]
    # an empty span is bad and frees nothing; span ends are clamped into the row
    odd = np.asarray([[-1, -1], [2, 1], [2, 900]], I32)
    pin, counts = R.repair_plan_ref(m[None], odd[None], [N], [0], [P], margin=0)
    assert counts[0].tolist() == [3, 2] and pin[0].tolist() == [1, 1, 0, 0]
    # rows without frames or without tokens: pin all 0, counts (0, 0)
    pin, counts = R.repair_plan_ref(np.stack([m2] * 3), np.stack([spans] * 3), [0, N, N], [0, 2, 3], [P, 2, 1], margin=0)
    assert not pin.any() and counts.tolist() == [[0, 0]] * 3


def test_keep_rule():
    inf, nan = np.inf, np.nan
    cur = np.asarray([2, 2, 2, nan, nan, inf, inf, 1, 1, 3], F32)
    new = np.asarray([1, 2, 3, 5, nan, inf, 7, nan, -inf, 1], F32)
    counts = np.asarray([[1, 4]] * 9 + [[1, 0]], I32)           # the last row: a lower total but nothing freed
    assert R.replace_ref(cur, new, counts).tolist() == [True, False, False, True, False, False, True, False, True, False]
    G, N, P = 10, 3, 2
    g = np.random.default_rng(0)
    x0, x1 = g.standard_normal((G, N, 64)).astype(F32), g.standard_normal((G, N, 64)).astype(F32)
    f0, f1 = np.zeros((G, 4), I32), np.ones((G, 4), I32)
    t, f, kept, x, sp, ms = R.repair_keep_ref(cur, new, counts, f0, f1, x0, x1)
    assert sp is None and ms is None and kept.tolist() == [1, 0, 0, 1, 0, 0, 1, 0, 1, 0]
    rep = kept.astype(bool)
    assert np.array_equal(x[rep], x1[rep]) and np.array_equal(x[~rep], x0[~rep]) and f[:, 0].tolist() == kept.tolist()
    assert t.tobytes() == np.where(rep, new, cur).astype(F32).tobytes()


def test_repair_settings():
    r = api.Repair()
    assert (r.rounds, r.tau_token, r.max_span, r.margin) == (1, 0.1, 8, 2)
    assert api.as_repair(None) is None and api.as_repair(1) == r and api.as_repair(r) is r and hash(r) == hash(api.Repair(1))
    assert api.as_repair(3).rounds == 3 and api.Repair(2, tau_token=0.3, max_span=225, margin=0) != api.Repair(2)
    with pytest.raises(AttributeError):
        r.rounds = 2
    for kw in (dict(rounds=0), dict(rounds=5), dict(max_span=0), dict(max_span=226), dict(margin=-1), dict(margin=33),
               dict(tau_token=float("nan")), dict(tau_token=float("inf"))):
        with pytest.raises(ValueError):
            api.Repair(**kw)
    for bad in (True, 2.0, "3"):
        with pytest.raises(TypeError):
            api.as_repair(bad)
    with pytest.raises(TypeError):
        api.Repair(max_span=8.0)
    # what is not known is said where a user reads it
    assert "UNVALIDATED on trained weights" in api.Repair.__doc__ and "not measurements" in api.Repair.__doc__


def test_repair_seeds():
    for s in (0, 1, 12345, 2 ** 62 + 7):
        rs = [api.repair_seed(s, r) for r in range(1, 5)]
        assert len(set(rs)) == 4 and s not in rs and all(0 <= v < 2 ** 63 for v in rs)
        assert not set(rs) & {api.take_seed(s, k) for k in range(16)}
        assert not set(rs) & {api.piece_seed(s, i) for i in range(16)}
    assert api.repair_seed(5, 1) == int(np.random.SeedSequence([5, 1, 0x52455052]).generate_state(1, np.uint64)[0] >> 1)
    with pytest.raises(ValueError):
        api.repair_seed(5, 0)


def test_the_entries_are_in_the_table_and_the_header():
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    norm = lambda s: [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in s.split(",")]
    for name, nargs in (("smtts_repair_plan", 16), ("smtts_repair_keep", 19)):
        assert name in _lib.SIGNATURES and name in _lib.header_symbols()
        res, args = _lib.SIGNATURES[name]
        decl = norm(re.search(rf"int {name}\(([^;]*)\);", txt).group(1))
        assert res is _lib.i32 and len(args) == len(decl) == nargs and args[0] is _lib.vp, name
        for a, d in zip(args, decl):
            assert (a is _lib.f32) == d.startswith("float ") and (a is _lib.i32) == d.startswith("int "), (name, d)
    assert re.search(r"#define\s+SMTTS_ABI_VERSION\s+(\d+)", txt).group(1) == str(_lib.ABI_VERSION) == "11"   # additive entries
    doc = txt[txt.index("---- repair"): txt.index("int smtts_repair_plan")]
    assert "UNVALIDATED on trained weights" in doc and "design" in doc and "not measurements" in doc


def test_the_synthesis_calls_take_repair():
    import inspect
    for fn in (api.SmallTTS.synthesize_batch, api.SmallTTS.synthesize_long):
        sig = inspect.signature(fn).parameters
        assert sig["repair"].default is None and sig["return_repair"].default is False
        assert "UNVALIDATED on trained weights" in fn.__doc__
    assert api._Batch._fields[-3:] == ("rp_kept", "rp_counts", "rp_totals") and api._Batch._field_defaults["rp_kept"] is None


def test_longform_repair_arguments(capsys):
    from smalltts_amd.scripts import longform as L
    base = ["--wav", "r.wav", "--tokens-file", "t.txt", "--durations", "1.0"]
    assert L.parse_args(base).repair is None
    assert L.parse_args(base + ["--repair"]).repair == 1          # the flag alone: one round
    assert L.parse_args(base + ["--repair", "3"]).repair == 3
    a = L.parse_args(base + ["--repair", "2", "--takes", "4"])
    assert (a.repair, a.takes) == (2, 4)
    for bad in ("0", "5", "x"):
        with pytest.raises(SystemExit):
            L.parse_args(base + ["--repair", bad])
    capsys.readouterr()
    words = [(0, "word", 0, 3200), (1, "punct", 3200, 6400)]
    texts = [(0, "word", "ab"), (0, "punct", ".")]
    mended = [(np.asarray([1, 0], I32), np.asarray([[2, 7], [1, 3]], I32), np.asarray([0.5, 0.25], F32), np.asarray([0.25, np.inf], F32))]
    doc = json.loads(L.words_json(words, texts, None, mended))
    assert doc["words"] == json.loads(L.words_json(words, texts)) and "takes" not in doc
    assert doc["repair"] == [{"piece": 0, "kept": [1, 0], "bad": [2, 1], "free": [7, 3], "before": [0.5, 0.25], "after": [0.25, None]}]
    chosen = [(2, 77, np.asarray([0.5, np.inf, 0.25], F32), np.zeros((3, 4), I32))]
    both = json.loads(L.words_json(words, texts, chosen, mended))
    assert both["takes"] == json.loads(L.words_json(words, texts, chosen))["takes"] and both["repair"] == doc["repair"]
