"""CPU: takes (best-of-K sampling): the numpy restatement of the two kernels on planted text-mass buffers, the selection
rule, the settings object, the seeds and the command line.  The GPU half (tests/test_takes_gpu.py) holds the kernels to this
restatement bit for bit."""
import json
import re

import numpy as np
import pytest

from smalltts_amd import _lib, api
from tests.helpers import takes_ref as T
from tests.helpers.align_ref import dp_align

F32 = np.float32


def scored(m, N, P, p0, **kw):
    spans, score, _path = dp_align(m, N, p0, P)
    feat, total = T.take_scores_ref(m[None], spans[None], [score], [N], [p0], [P], **kw)
    return feat[0].tolist(), float(total[0])


@pytest.fixture(scope="module")
def planted_scores():
    """{(N, P, p0): {variant: (features, total)}}, computed once."""
    return {s: {v: scored(T.planted(*s, v), *s) for v in T.VARIANTS} for s in T.SHAPES}


@pytest.mark.parametrize("shape", T.SHAPES)
def test_clean_wins_and_the_features_move_as_planted(planted_scores, shape):
    N, P, p0 = shape
    r = planted_scores[shape]
    (cells, skipped, longest, idle), clean = r["clean"]
    assert (skipped, idle) == (0, 0) and cells >= N and longest <= -(-N // (P - p0)) + 1
    for v in ("skip", "stall", "idle"):
        assert clean < r[v][1], (v, clean, r[v][1])
    assert r["skip"][0][1] >= 1 and r["skip"][0][3] == 0                    # a token nobody attends to, no idle frame
    assert r["stall"][0][2] >= 2 * longest and r["stall"][0][1] == 0         # one long span, every token still spoken
    assert r["idle"][0][3] == N // 5                                        # exactly the frames that were blanked
    # the selection over the four takes in the order of the GPU test: (stall, skip, clean, idle) -> k = 2
    totals = np.asarray([r[v][1] for v in ("stall", "skip", "clean", "idle")], F32)
    assert T.winners_ref(totals, 4).tolist() == [2]


def test_selection_rule():
    inf, nan = np.inf, np.nan
    total = np.asarray([3, 1, 1, 2,          # a tie: the lowest k
                        nan, 5, inf, 7,      # NaN counts as +inf
                        inf, inf, inf, inf,  # nothing finite: k = 0
                        nan, nan, nan, nan,
                        2, nan, 1, 1], F32)
    assert T.winners_ref(total, 4).tolist() == [1, 1, 0, 0, 2]
    assert T.winners_ref(total[:4], 1).tolist() == [0, 0, 0, 0]
    x = np.arange(20 * 3 * 64, dtype=F32).reshape(20, 3, 64)
    xw, nw, sw, mw, win = T.take_select_ref(total, 4, x, list(range(20)))
    assert sw is None and mw is None and nw.tolist() == [1, 5, 8, 12, 18] and np.array_equal(xw, x[[1, 5, 8, 12, 18]])


def test_a_value_at_the_threshold_attends_and_a_nan_does_not():
    N, P = 4, 3
    tau = F32(0.1)
    below = np.nextafter(tau, F32(0))
    m = np.full((N, P), below, F32)
    spans = np.asarray([[0, 0], [1, 2], [3, 3]], np.int32)
    args = (spans[None], [F32(2.0)], [N], [0], [P])
    feat, total = T.take_scores_ref(m[None], *args)
    assert feat[0].tolist() == [4, 3, 2, 4]                     # nothing reaches the threshold: all skipped, all idle
    m2 = m.copy()
    m2[0, 0] = m2[2, 1] = m2[3, 2] = tau                        # exactly at it: attended
    feat, total = T.take_scores_ref(m2[None], *args)
    assert feat[0].tolist() == [4, 0, 2, 1]                     # frame 1 alone stays idle
    want = F32(F32(F32(2.0) / F32(4)) + F32(F32(2.0) * F32(0.0)))
    want = F32(F32(want + F32(F32(2) / F32(4))) + F32(F32(1) / F32(4)))
    assert total[0] == want
    m3 = m2.copy()
    m3[0, 0] = np.nan                                           # a NaN satisfies no comparison
    feat, _ = T.take_scores_ref(m3[None], *args)
    assert feat[0].tolist() == [4, 1, 2, 2]
    # empty rows: features 0, total +inf; a span off the path is empty and skipped; span ends are clamped into the row
    feat, total = T.take_scores_ref(np.stack([m2, m2, m2]), np.stack([spans] * 3), [F32(1)] * 3, [0, N, N], [0, 2, 0], [P, 2, P])
    assert feat[:2].tolist() == [[0] * 4] * 2 and np.isposinf(total[:2]).all()
    odd = np.asarray([[-1, -1], [2, 1], [2, 900]], np.int32)
    feat, _ = T.take_scores_ref(m2[None], odd[None], [F32(1)], [N], [0], [P])
    assert feat[0].tolist() == [2, 2, 2, 1]


def test_takes_settings():
    t = api.Takes(3)
    assert (t.k, t.weights, t.tau_token, t.tau_frame) == (3, (1.0, 2.0, 1.0, 1.0), 0.1, 0.1)
    assert api.as_takes(None) is None and api.as_takes(3) == t and api.as_takes(t) is t and hash(t) == hash(api.Takes(3))
    assert api.Takes(2, weights=(0, 1, 0, 0), tau_token=0.3) != api.Takes(2)
    with pytest.raises(AttributeError):
        t.k = 4
    for bad in (0, 17, -1):
        with pytest.raises(ValueError):
            api.Takes(bad)
    for kw in (dict(weights=(1, 2, 3)), dict(weights=(1, -1, 1, 1)), dict(weights=(1, float("nan"), 1, 1)), dict(tau_token=float("nan")),
               dict(tau_frame=float("inf"))):
        with pytest.raises(ValueError):
            api.Takes(2, **kw)
    for bad in (True, 2.0, "3"):
        with pytest.raises(TypeError):
            api.as_takes(bad)
    # what is not known is said where a user reads it
    assert "UNVALIDATED on trained weights" in api.Takes.__doc__ and "not measurements" in api.Takes.__doc__


def test_take_seeds():
    for s in (0, 1, 12345, 2 ** 62 + 7):
        assert api.take_seed(s, 0) == s
        ks = [api.take_seed(s, k) for k in range(1, 16)]
        assert len(set(ks)) == 15 and s not in ks and all(0 <= v < 2 ** 63 for v in ks)
        assert not set(ks) & {api.piece_seed(s, i) for i in range(16)}
    assert api.take_seed(5, 1) == int(np.random.SeedSequence([5, 1, 0x54414B45]).generate_state(1, np.uint64)[0] >> 1)


def test_the_entries_are_in_the_table_and_the_header():
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    norm = lambda s: [" ".join(re.sub(r"/\*.*?\*/", "", a).split()) for a in s.split(",")]
    for name, nargs in (("smtts_take_scores", 19), ("smtts_take_select", 16)):
        assert name in _lib.SIGNATURES and name in _lib.header_symbols()
        res, args = _lib.SIGNATURES[name]
        decl = norm(re.search(rf"int {name}\(([^;]*)\);", txt).group(1))
        assert res is _lib.i32 and len(args) == len(decl) == nargs and args[0] is _lib.vp, name
        for a, d in zip(args, decl):
            assert (a is _lib.f32) == d.startswith("float ") and (a is _lib.i32) == d.startswith("int "), (name, d)
    assert re.search(r"#define\s+SMTTS_ABI_VERSION\s+(\d+)", txt).group(1) == str(_lib.ABI_VERSION)
    doc = txt[txt.index("---- takes"): txt.index("int smtts_take_scores")]
    assert "UNVALIDATED on trained weights" in doc and "design" in doc and "not measurements" in doc


def test_longform_takes_arguments(capsys):
    from smalltts_amd.scripts import longform as L
    base = ["--wav", "r.wav", "--tokens-file", "t.txt", "--durations", "1.0"]
    a = L.parse_args(base)
    assert a.takes is None and a.max_batch == 8
    a = L.parse_args(base + ["--takes", "4"])
    assert a.takes == 4 and a.max_batch == 8
    a = L.parse_args(base + ["--takes", "1"])                   # one take: accepted (main reports winner 0 per piece)
    assert a.takes == 1 and a.max_batch == 8
    a = L.parse_args(base + ["--takes", "16"])
    assert a.takes == 16 and a.max_batch == 4                   # 64 sampler rows at the most: the group shrinks, and --take records it
    for bad in ("0", "17", "x"):
        with pytest.raises(SystemExit):
            L.parse_args(base + ["--takes", bad])
    capsys.readouterr()
    words = [(0, "word", 0, 3200), (1, "punct", 3200, 6400)]
    texts = [(0, "word", "ab"), (0, "punct", ".")]
    assert isinstance(json.loads(L.words_json(words, texts)), list)          # without --takes: the list it always was
    chosen = [(2, 77, np.asarray([0.5, np.inf, 0.25], F32), np.zeros((3, 4), np.int32))]
    doc = json.loads(L.words_json(words, texts, chosen))
    assert doc["words"] == json.loads(L.words_json(words, texts))
    assert doc["takes"] == [{"piece": 0, "winner": 2, "seed": 77, "totals": [0.5, None, 0.25]}]
