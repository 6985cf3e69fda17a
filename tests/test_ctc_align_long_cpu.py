"""CPU: the host side of long alignment.  The vectorised restatement (tests/helpers/ctc_align_long_ref.py) is held to
tests/helpers/ctc_align_ref.align on 200 seeded ragged rows, bit for bit, the state sequence included; the window table of
asr_logprobs_long and plans.speaking_rate on hand-worked values; the new HipEngine methods against the stand-in library
(tests/helpers/engine_standin.py): the C calls they make, and every host-side refusal reached with exactly one thing wrong; the two new
names in the signature table and the header."""
import numpy as np
import pytest
import torch

import smalltts_amd.engine  # noqa: F401  (loaded before the stand-in patches its _p)
from smalltts_amd import _lib
from smalltts_amd.plans import long_windows, speaking_rate
from tests.helpers import ctc_align_long_ref as L
from tests.helpers import ctc_align_ref as R
from tests.helpers.engine_standin import record


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


def test_the_vectorised_restatement_equals_the_definition_on_200_ragged_rows():
    rng = np.random.default_rng(2024)
    seen = dict(aligned=0, infeasible=0, empty=0, nan_score=0, window=0)
    for i in range(200):
        T, C, P = int(rng.integers(1, 48)), int(rng.integers(2, 9)), int(rng.integers(1, 12))
        lp = np.log(rng.dirichlet(np.ones(C), size=T)).astype(np.float32)
        if i % 3 == 0:
            lp = (np.round(lp * 4.0) / 4.0).astype(np.float32)             # quantised: ties everywhere
        if i % 5 == 0:
            lp[rng.integers(0, T, 3), rng.integers(0, C, 3)] = -np.inf
        if i % 7 == 0:
            lp[rng.integers(0, T), rng.integers(0, C)] = np.nan
        tok = rng.integers(-1, C + 2, P)                                    # 0, negative and >= C: clamped
        if i % 4 == 0:
            tok[:] = tok[0]                                                 # repeats: a blank between every pair
        t_len = int(rng.integers(0, T + 3)) if i % 6 else 0
        p0, p1 = (int(rng.integers(-2, P + 1)), int(rng.integers(0, P + 3))) if i % 2 else (0, P)
        if i % 11 == 0:
            p1 = p0                                                         # L = 0
        a, b = R.align(lp, t_len, tok, p0, p1), L.align(lp, t_len, tok, p0, p1)
        assert np.array_equal(a["spans"], b["spans"]) and a["spans"].dtype == b["spans"].dtype, i
        assert np.array_equal(a["frame_tok"], b["frame_tok"]) and a["frame_tok"].dtype == b["frame_tok"].dtype, i
        assert same_bits(a["tok_logp"], b["tok_logp"]) and same_bits(a["score"], b["score"]), i
        assert (a["state"] is None) == (b["state"] is None), i
        if a["state"] is not None:
            assert list(a["state"]) == [int(s) for s in b["state"]], i
            seen["aligned"] += 1
            seen["window"] += (p0, p1) != (0, P)
        elif t_len <= 0 or min(max(p1, 0), P) - min(max(p0, 0), P) <= 0:
            seen["empty"] += 1
        elif np.isnan(a["score"]):
            seen["nan_score"] += 1
        else:
            seen["infeasible"] += 1
    assert seen["aligned"] >= 40 and seen["infeasible"] >= 5 and seen["empty"] >= 20 and seen["window"] >= 10, seen


def test_the_batch_form_stacks_the_rows():
    rng = np.random.default_rng(1)
    lp = np.log(rng.dirichlet(np.ones(5), size=(3, 20))).astype(np.float32)
    tok = rng.integers(1, 5, (3, 6))
    a, b = R.align_batch(lp, [20, 14, 0], tok, [0, 1, 0], [6, 6, 6]), L.align_batch(lp, [20, 14, 0], tok, [0, 1, 0], [6, 6, 6])
    assert all(x.dtype == y.dtype and x.shape == y.shape and (same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y))
               for x, y in zip(a, b))


# ---- the window table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 225, 226, 404, 405, 406, 16384])
def test_window_table(N):
    W, H = 225, 180
    starts, cuts, src = long_windows(N)
    n_w = len(starts)
    assert n_w == (1 if N <= W else 1 + -(-(N - W) // H)) and len(cuts) == n_w + 1 and cuts[0] == 0 and cuts[-1] == N
    assert src.shape == (N,) and src.dtype == np.int32
    cover = np.zeros(N, np.int64)
    for w in range(n_w):
        assert cuts[w] < cuts[w + 1]                                        # every window gives at least one frame
        cover[cuts[w]:cuts[w + 1]] += 1
        assert (src[cuts[w]:cuts[w + 1]] == w).all()
        assert starts[w] <= cuts[w] and cuts[w + 1] <= starts[w] + min(W, N)      # its frames lie inside it
        if N > W:
            assert 0 <= starts[w] and starts[w] + W <= N                    # every window is full
    assert (cover == 1).all()                                               # every frame exactly once
    for w in range(1, n_w):                                                 # every cut lies inside both windows
        assert starts[w] <= cuts[w] <= starts[w - 1] + W and starts[w - 1] < starts[w]
        assert cuts[w] == (starts[w - 1] + W + starts[w]) // 2


def test_window_table_hand_worked_values():
    assert long_windows(1)[:2] == ([0], [0, 1]) and long_windows(225)[:2] == ([0], [0, 225])
    assert long_windows(226)[:2] == ([0, 1], [0, 113, 226])
    assert long_windows(404)[:2] == ([0, 179], [0, 202, 404])
    assert long_windows(405)[:2] == ([0, 180], [0, 202, 405])
    assert long_windows(406)[:2] == ([0, 180, 181], [0, 202, 293, 406])
    starts, cuts, _ = long_windows(16384)
    assert len(starts) == 91 and starts[:3] == [0, 180, 360] and starts[-2:] == [16020, 16159] and cuts[-2] == (16020 + 225 + 16159) // 2
    with pytest.raises(ValueError, match="long_windows"):
        long_windows(0)


# ---- speaking rate ----------------------------------------------------------------------------------------------------------------------
def test_speaking_rate_hand_worked():
    nan_zero = lambda r: r[0] != r[0] and r[1] == 0.0
    # three tokens on frames 0-3, 4-5, 20-21: the gap of 14 frames counts as 6 -> 4 + 2 + 6 + 2 = 14 frames = 14 / 30 s
    rate, sec = speaking_rate([[0, 3], [4, 5], [20, 21], [-1, -1]])
    assert sec == 14 * 800 / 24000 and rate == 3 / sec
    # a gap of exactly max_pause is kept whole; one more is capped
    assert speaking_rate([[10, 10], [17, 17]]) == (2 / (8 / 30), 8 / 30)
    assert speaking_rate([[10, 10], [18, 18]]) == (2 / (8 / 30), 8 / 30)
    assert speaking_rate([[10, 10], [18, 18]], max_pause=7) == (2 / (9 / 30), 9 / 30)
    assert speaking_rate([[10, 10], [18, 18]], max_pause=0) == (2 / (2 / 30), 2 / 30)
    # tokens off the path are left out, leading and trailing silence never counts
    assert speaking_rate([[-1, -1], [100, 101], [-1, -1], [102, 103], [-1, -1]]) == (2 / (4 / 30), 4 / 30)
    assert nan_zero(speaking_rate([[5, 9]])) and nan_zero(speaking_rate(np.full((4, 2), -1))) and nan_zero(speaking_rate(np.zeros((0, 2))))
    for bad in ([1, 2, 3], np.zeros((3, 3))):
        with pytest.raises(ValueError, match="speaking_rate"):
            speaking_rate(bad)
    with pytest.raises(ValueError, match="max_pause"):
        speaking_rate([[0, 1], [2, 3]], max_pause=-1)


def test_encoder_lookback_hand_worked():
    from smalltts_amd.plans import encoder_lookback
    from smalltts_amd.weights import DEFAULT_CODEC as spec
    assert encoder_lookback(7, (), (1,)) == 6 + 6 + 6                       # stem, one block, head, all at the sample rate
    assert encoder_lookback(3, (2,), (0, 1)) == 2 + 2 + 2 * 2 + 2 * 2       # stem 2; down 2 x 1; one block 2 x 2; head 2 x 2
    got = encoder_lookback(spec.kernel, spec.enc_ratios, spec.enc_depths)
    assert got == 185562 and -(-got // spec.hop) == 58                      # 32 frames of context are 26 short of it


# ---- HipEngine against the stand-in library -----------------------------------------------------------------------------------------------
B, T, P, CN = 2, 8, 5, 7
ts, p0, p1 = [8, 6], [0, 1], [5, 4]


def ops(**kw):
    import types
    base = dict(logp=torch.zeros(B, T, CN), tokens=torch.ones(B, P, dtype=torch.int32))
    base.update(kw)
    return types.SimpleNamespace(**base)


def made(lib):
    """the C calls of a section by name (an engine collected in the meantime adds its smtts_destroy: not the method's)"""
    return [name for name, _ in lib.calls if name != "smtts_destroy"]


def test_ctc_align_long_makes_the_size_query_and_one_launch():
    for frames in (False, True):
        lines, lib = record("ctc_align_long", lambda e, o: e.ctc_align_long(o.logp, ts, o.tokens, p0, p1, frames=frames), ops())
        assert lib.error is None
        assert made(lib) == ["smtts_ctc_align_long_workspace_bytes", "smtts_ctc_align_long"]
        assert lines[1] == "smtts_ctc_align_long_workspace_bytes h 2 8 5"
        ft = "ret[3]+0" if frames else "null"
        assert lines[2] == ("smtts_ctc_align_long h stream logp+0 table0+0 tokens+0 table0+8 table0+16 2 8 5 7 ret[0]+0 ret[1]+0 "
                            f"{ft} ret[2]+0 ws+0 256")
        assert lines[3] == "table0 int32(3, 2) [[8, 6], [0, 1], [5, 4]]"
        assert lines[4] == ("-> (int32(2, 5, 2), float32(2, 5), float32(2,)" + (", int32(2, 8))" if frames else ")"))


REFUSED = [
    ("logp fp64", lambda e, o: e.ctc_align_long(o.logp.double(), ts, o.tokens, p0, p1), "ctc_align_long: logp"),
    ("logp not contiguous", lambda e, o: e.ctc_align_long(torch.zeros(B, T, 2 * CN)[:, :, ::2], ts, o.tokens, p0, p1), "ctc_align_long: logp"),
    ("logp 2-d", lambda e, o: e.ctc_align_long(o.logp[0], ts, o.tokens, p0, p1), "ctc_align_long: logp"),
    ("logp on another device", lambda e, o: e.ctc_align_long(o.logp.to("meta"), ts, o.tokens, p0, p1), "ctc_align_long: logp"),
    ("tokens int64", lambda e, o: e.ctc_align_long(o.logp, ts, o.tokens.long(), p0, p1), "ctc_align_long: tokens"),
    ("tokens rows", lambda e, o: e.ctc_align_long(o.logp, ts, torch.ones(3, P, dtype=torch.int32), p0, p1), "ctc_align_long: tokens"),
    ("T 65537", lambda e, o: e.ctc_align_long(torch.zeros(1, 65537, 2), [5], o.tokens[:1], [0], [4]), "1 <= T <= 65536, P <= 16383"),
    ("P 16384", lambda e, o: e.ctc_align_long(o.logp, ts, torch.ones(B, 16384, dtype=torch.int32), p0, p1), "1 <= T <= 65536, P <= 16383"),
    ("C 1", lambda e, o: e.ctc_align_long(torch.zeros(B, T, 1), ts, o.tokens, p0, p1), "2 <= C <= 256"),
    ("C 257", lambda e, o: e.ctc_align_long(torch.zeros(B, T, 257), ts, o.tokens, p0, p1), "2 <= C <= 256"),
    ("B 65", lambda e, o: e.ctc_align_long(torch.zeros(65, 2, 2), [2] * 65, torch.ones(65, 1, dtype=torch.int32), [0] * 65, [1] * 65),
     "at most 64"),
    ("one ts", lambda e, o: e.ctc_align_long(o.logp, [8], o.tokens, p0, p1), "one frame count"),
    ("one p1", lambda e, o: e.ctc_align_long(o.logp, ts, o.tokens, p0, [4]), "one frame count"),
    ("x fp64", lambda e, o: e.asr_logprobs_long(torch.zeros(5, 64, dtype=torch.float64)), "asr_logprobs_long: x"),
    ("x 3-d", lambda e, o: e.asr_logprobs_long(torch.zeros(1, 5, 64)), "asr_logprobs_long: x"),
    ("x 63 wide", lambda e, o: e.asr_logprobs_long(torch.zeros(5, 63)), "asr_logprobs_long: x"),
    ("x not contiguous", lambda e, o: e.asr_logprobs_long(torch.zeros(5, 128)[:, ::2]), "asr_logprobs_long: x"),
    ("N 0", lambda e, o: e.asr_logprobs_long(torch.zeros(0, 64)), "1 <= N <= 16384"),
    ("N 16385", lambda e, o: e.asr_logprobs_long(torch.zeros(16385, 64)), "1 <= N <= 16384"),
    ("max_rows 0", lambda e, o: e.asr_logprobs_long(torch.zeros(5, 64), max_rows=0), "max_rows"),
    ("max_rows 65", lambda e, o: e.asr_logprobs_long(torch.zeros(5, 64), max_rows=65), "max_rows"),
]


@pytest.mark.parametrize("title,fn,text", REFUSED, ids=[r[0] for r in REFUSED])
def test_every_host_side_refusal_with_one_thing_wrong(title, fn, text):
    lines, lib = record("refused: " + title, fn, ops())
    assert isinstance(lib.error, ValueError) and text in str(lib.error), lines[-1]
    assert not made(lib)                                                   # not even a size query


def test_the_librarys_own_refusal_and_a_missing_recogniser_are_reported():
    lines, lib = record("library says no", lambda e, o: e.ctc_align_long(o.logp, ts, o.tokens, p0, p1), ops(), fail=("smtts_ctc_align_long",))
    assert isinstance(lib.error, RuntimeError) and "ctc_align_long: stand-in text" in str(lib.error)
    lines, lib = record("no recogniser", lambda e, o: e.asr_logprobs_long(torch.zeros(300, 64)), ops(), parts=0)
    assert isinstance(lib.error, ValueError) and "recogniser" in str(lib.error)
    assert not [n for n in made(lib) if n != "smtts_has_part"]


def test_asr_logprobs_long_calls_the_recogniser_window_by_window():
    # one window: asr_logprobs itself, the bits of that call
    lines, lib = record("short", lambda e, o: e.asr_logprobs_long(o.x), ops(x=torch.zeros(40, 64)))
    assert lib.error is None and [n for n, _ in lib.calls if n == "smtts_asr_logprobs"] == ["smtts_asr_logprobs"]
    call = next(a for n, a in lib.calls if n == "smtts_asr_logprobs")
    assert call[4:6] == ["1", "40"] and lines[-1] == "-> float32(160, 198)"
    assert any(l.startswith("smtts_asr_logprobs h stream x+0 ") for l in lines)            # the caller's own buffer, no copy
    # 406 frames: three full windows, all in one call; with max_rows = 2 two calls of two rows and one
    for max_rows, rows in ((64, ["3"]), (2, ["2", "1"]), (1, ["1", "1", "1"])):
        lines, lib = record("long", lambda e, o: e.asr_logprobs_long(o.x, max_rows=max_rows), ops(x=torch.zeros(406, 64)))
        assert lib.error is None and lines[-1] == "-> float32(1624, 198)"
        calls = [a for n, a in lib.calls if n == "smtts_asr_logprobs"]
        assert [a[4] for a in calls] == rows and all(a[5] == "225" for a in calls)
        tables = [l for l in lines if l.startswith("table")]
        assert tables == [f"table{i} int32(1, {r}) [[{', '.join(['225'] * int(r))}]]" for i, r in enumerate(rows)]
    # the windows handed over are the table's: x[a_w : a_w + 225]
    seen = []
    x = torch.arange(406, dtype=torch.float32)[:, None].repeat(1, 64).contiguous()

    def run(e, o):
        inner = e.asr_logprobs
        def spy(xs, ns, out=None):
            seen.append(xs[:, :, 0].clone())
            return inner(xs, ns, out)
        e.asr_logprobs = spy
        return e.asr_logprobs_long(o.x)
    record("windows", run, ops(x=x))
    assert len(seen) == 1 and seen[0].shape == (3, 225)
    assert [int(r[0]) for r in seen[0]] == [0, 180, 181] and [int(r[-1]) for r in seen[0]] == [224, 404, 405]


# ---- the C ABI tables -----------------------------------------------------------------------------------------------------------------
def test_signature_table_and_header_hold_both_names():
    syms = _lib.header_symbols()
    for name in ("smtts_ctc_align_long", "smtts_ctc_align_long_workspace_bytes"):
        assert name in _lib.SIGNATURES and name in syms
    assert _lib.ABI_VERSION == 11
    assert len(_lib.SIGNATURES["smtts_ctc_align_long"][1]) == 17 == len(_lib.SIGNATURES["smtts_ctc_align"][1]) + 2
    assert _lib.SIGNATURES["smtts_ctc_align_long"][1][:15] == _lib.SIGNATURES["smtts_ctc_align"][1]
    assert _lib.SIGNATURES["smtts_ctc_align_long"][1][15:] == [_lib.vp, _lib.sz] and _lib.SIGNATURES["smtts_ctc_align_long"][0] is _lib.i32
    assert _lib.SIGNATURES["smtts_ctc_align_long_workspace_bytes"] == (_lib.sz, [_lib.vp, _lib.i32, _lib.i32, _lib.i32])
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    decl = txt[txt.index("int smtts_ctc_align_long("):]
    assert len(decl[:decl.index(");")].split(",")) == 17
