"""GPU: pitch (include/smalltts_hip.h smtts_pitch).  The two kernels against the numpy restatement of
tests/helpers/pitch_ref.py: the scores within the derived bound of the float64 scores, per element; the path teacher-forced (the
reference path run on the DEVICE's own scores) and bit for bit; free-running, the conditions tests/test_pitch_cpu.py holds the reference
to; the retime / pitch yardstick; determinism, row independence, NaN, guard bands, refusals; and the public layers on top.  Synthetic
signals only; no tolerance here is a tuned number."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from smalltts_amd import options, plans
from tests.helpers import pitch_ref as R
from tests.helpers import retime_ref as RT
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
SENTINEL, LAG_SENTINEL = 7.25, -77


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    from tests.test_stream_gpu import API_SEED, API_SPEC
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(API_SEED, parts=("dit", "decoder", "encoder"), codec_spec=API_SPEC)
    e.finalize()
    return e


def _ws_bytes(eng, B, S, P):
    need = int(eng.lib.smtts_pitch_workspace_bytes(eng.h, B, S, P.hop, P.lmin, P.lmax))
    assert need > 0, eng.lib.smtts_last_error(eng.h)
    return need


def _pack(rows, P, row_stride=None, behind=0.0):
    """Rows (x, len) -> the host arrays of one call: audio (B,1,S) with `behind` behind every len, len."""
    S = max(x.size for x, _n in rows) if row_stride is None else row_stride
    audio = np.full((len(rows), 1, S), behind, np.float32)
    for b, (x, n) in enumerate(rows):
        m = max(0, min(int(n), x.size, S))
        audio[b, 0, :m] = x[:m]
    return dict(audio=audio, len=np.asarray([n for _x, n in rows], np.int64), S=S, Fmax=-(-S // P.hop))


def _launch(eng, d, P, t, nccf=True, **over):
    a = dict(audio=_p(t["audio"]), B=d["audio"].shape[0], row_stride=d["S"], len=_p(t["len"]), tab=_p(t["tab"]), hop=P.hop, win=P.win,
             lmin=P.lmin, lmax=P.lmax, bias=float(P.bias), c_unv=float(P.c_unv), w_jump=float(P.w_jump), w_switch=float(P.w_switch),
             lag=_p(t["lag"]), peak=_p(t["peak"]), nccf=_p(t["nccf"]) if nccf else None, ws=_p(t["ws"]), ws_bytes=int(t["ws"].numel()))
    a.update(over)
    return eng.lib.smtts_pitch(eng.h, eng._stream(), a["audio"], a["B"], a["row_stride"], a["len"], a["tab"], a["hop"], a["win"], a["lmin"],
                               a["lmax"], a["bias"], a["c_unv"], a["w_jump"], a["w_switch"], a["lag"], a["peak"], a["nccf"], a["ws"],
                               a["ws_bytes"])


def _call(eng, rows, P, nccf=True, tab=None, **kw):
    """One call on plain tensors -> (lag (B,Fmax), peak (B,Fmax,3), nccf (B,Fmax,L) or None), each filled with its sentinel first."""
    d = _pack(rows, P, **kw)
    B = len(rows)
    t = {k: torch.from_numpy(d[k]).to(eng.device) for k in ("audio", "len")}
    t["tab"] = torch.from_numpy(P.tab if tab is None else tab).to(eng.device)
    t["lag"] = torch.full((B, d["Fmax"]), LAG_SENTINEL, dtype=torch.int32, device=eng.device)
    t["peak"] = torch.full((B, d["Fmax"], 3), SENTINEL, device=eng.device)
    t["nccf"] = torch.full((B, d["Fmax"], P.L), SENTINEL, device=eng.device) if nccf else None
    t["ws"] = torch.empty(_ws_bytes(eng, B, d["S"], P), dtype=torch.uint8, device=eng.device)
    assert _launch(eng, d, P, t, nccf=nccf) == 0, eng.lib.smtts_last_error(eng.h)
    return t["lag"].cpu().numpy(), t["peak"].cpu().numpy(), (t["nccf"].cpu().numpy() if nccf else None)


def _frames(P, x, n, S=None):
    return P.frames(min(max(int(n), 0), x.size if S is None else S))


def _judge(name, P, rows, lag, peak, nccf, S=None, tab=None, scores=True):
    """Every row of a call: nothing at or behind F_b; the scores within the derived bound; the reference path on the device's own
    scores equals lag, and peak equals the copies out of nccf, bit for bit."""
    worst = 0.0
    for b, (x, n) in enumerate(rows):
        F = _frames(P, x, n, S)
        assert (lag[b, F:] == LAG_SENTINEL).all() and (peak[b, F:] == SENTINEL).all() and (nccf[b, F:] == SENTINEL).all(), (name, b)
        if scores:
            S64, E = R.scores(x, n, P, row_stride=S)
            err = np.abs(nccf[b, :F].astype(np.float64) - S64)
            assert (err <= E).all(), (name, b, float((err - E).max()), np.unravel_index(np.argmax(err - E), err.shape))
            worst = max(worst, float((err / np.maximum(E, 1e-300)).max()) if F else 0.0)
        want_lag, want_peak = R.path(nccf[b, :F], P, tab=tab)
        assert np.array_equal(lag[b, :F], want_lag), (name, b, np.flatnonzero(lag[b, :F] != want_lag)[:5])
        assert np.array_equal(_bits(peak[b, :F]), _bits(want_peak)), (name, b)
    return worst


# ---- the signals of each shape ----------------------------------------------------------------------------------------------------------
def _burst(n, a, b, seed):
    x = np.zeros((n,), np.float32)
    x[a:b] = 0.9 * np.random.default_rng(seed).uniform(-1, 1, b - a).astype(np.float32)
    return x


def _signals(name):
    """A tone with silent ends, noise, silence (exactly 0) and a loud burst between silences, at the shape's smallest useful length."""
    if name == "default":                                        # rows of 0.5 s
        n = 12000
        return [R.tone(220.0, n, 1200, 10800, None, seed=2), R.white(3, n), np.zeros((n,), np.float32), _burst(n, 5000, 6500, 4)]
    if name == "tiny":
        n = R.TINY_N
        return [R.tiny_case(13), R.white(3, n), np.zeros((n,), np.float32), _burst(n, 700, 900, 4)]
    n = 800                                                      # wide: 50 frames of 1023 lags
    return [R.periodic(300, n + 1100, 100, n + 1100, seed=5)[:n], R.white(3, n), np.zeros((n,), np.float32), _burst(n, 500, 700, 4)]


def _odd_rows(name, P):
    """B = 3: len = 0, len < win, len no multiple of hop."""
    sig = _signals(name)
    return [(sig[0], 0), (sig[1], P.win - 3), (sig[0], sig[0].size - P.hop // 2 - 1)]


# ---- 1. scores within the bound, 2. the path teacher-forced -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_scores_lie_within_the_derived_bound_and_the_path_is_the_references_bit_for_bit(eng, name):
    P = R.SHAPES[name]
    rows = [(x, x.size) for x in _signals(name)]
    lag, peak, nccf = _call(eng, rows, P)
    worst = _judge(name, P, rows, lag, peak, nccf)
    print(f"{name}: worst score error {worst:.3f} of its bound; voiced frames per row {[(l > 0).sum() for l in lag]}")
    F = P.frames(rows[2][0].size)
    assert not nccf[2, :F].any() and not lag[2, :F].any() and not peak[2, :F].any()          # silence: exactly 0 in, exactly 0 out
    assert (lag[0] > 0).sum() >= 10                                                           # the tone row is tracked at all


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_odd_lengths_and_a_single_frame(eng, name):
    P = R.SHAPES[name]
    rows = _odd_rows(name, P)
    lag, peak, nccf = _call(eng, rows, P)
    _judge(name, P, rows, lag, peak, nccf)
    assert (lag[0] == LAG_SENTINEL).all() and (peak[0] == SENTINEL).all() and (nccf[0] == SENTINEL).all()   # F_b = 0 writes nothing
    assert P.frames(rows[2][1]) * P.hop != rows[2][1]
    x = _signals(name)[0]
    for n in (1, P.hop - 1, P.hop):                              # one frame only
        one = [(x[x.size // 2:], n)]
        lag, peak, nccf = _call(eng, one, P, row_stride=P.hop)
        assert lag.shape == (1, 1)
        _judge(f"{name} one frame of {n}", P, one, lag, peak, nccf, S=P.hop)


# ---- 2b. ties on the path: the smallest state wins, whatever the split of the predecessors ----------------------------------------------
TIE_SHAPES = {"tiny": R.Shape(hop=16, win=64, lmin=8, lmax=40, c_unv=2.0),       # 4 shares of the predecessors
              "default": R.Shape(c_unv=2.0)}                                     # 2 shares


def _tie_rows(P):
    """A constant row: r, e and e0 of an inner frame are the same products in the same order at every lag, so S[f][l] is bit-equal
    across the lags.  A silent row: S = 0 everywhere, also in the last frame.  With a flat table (lg all equal, tilt all 1) every voiced
    state then costs the same, and with c_unv = 2 even the silent row is voiced: every minimum of every frame is a tie of all L voiced
    states, in the recurrence and (the silent row) at the end."""
    n = 40 * P.hop + P.reach
    return [(np.full((n,), 0.5, np.float32), n), (np.zeros((n,), np.float32), n), (np.full((n,), 0.5, np.float32), n - P.hop // 2 - 1)]


def _flat_table(P):
    return np.stack([np.zeros((P.L,), np.float32), np.ones((P.L,), np.float32)])


@pytest.mark.parametrize("name", sorted(TIE_SHAPES))
def test_ties_on_the_path_go_to_the_smallest_state(eng, name):
    P = TIE_SHAPES[name]
    rows, flat = _tie_rows(P), _flat_table(P)
    lag, peak, nccf = _call(eng, rows, P, tab=flat)
    _judge(f"ties {name}", P, rows, lag, peak, nccf, tab=flat)                    # the reference path on these scores, bit for bit
    for b, (x, n) in enumerate(rows):
        F = P.frames(n)
        inner = R.inside(P, n, [(0, n)]) if b != 1 else np.ones((F,), bool)
        assert inner.sum() >= 30
        assert (nccf[b, :F][inner] == nccf[b, :F][inner][:, :1]).all(), b         # the scores do tie, bit for bit
        assert (lag[b, :F][inner] == P.lmin).all(), (b, lag[b, :F])
        other = R.path(nccf[b, :F], P, tab=flat, ties="largest")[0]               # ... and the case can tell the rules apart
        assert (other[inner][:-1] != P.lmin).all(), b
    assert (lag[1, :P.frames(rows[1][1])] == P.lmin).all()                        # the silent row: the end rule too


# ---- 3. free-running: the conditions of the CPU file on device output ---------------------------------------------------------------------
def test_tones_silence_and_noise_at_the_defaults(eng):
    P = R.DEFAULT
    rows = [(R.tone_case(f0), R.TONE_N) for f0 in R.TONES] + [(R.white(5, 24000), 24000)]
    lag, peak, nccf = _call(eng, rows, P)
    for b, f0 in enumerate(R.TONES):
        R.check_tone(lag[b], P, R.TONE_N, R.TONE_ON, R.TONE_OFF, R.TONE_HOLE, R.SR / f0)
    assert (lag[4, :100] == 0).all()                             # white noise has no voiced frame
    f, strength = plans.pitch_f0(lag[1, :150], peak[1, :150])
    inner = R.inside(P, R.TONE_N, [(R.TONE_ON, R.TONE_HOLE[0]), (R.TONE_HOLE[1], R.TONE_OFF)])
    assert (np.abs(f[inner] - 100.0) <= 100.0 ** 2 / R.SR).all() and (strength[inner] > 0.9).all()


def test_the_long_tone_keeps_its_octave(eng):
    from tests.test_pitch_cpu import LONG_390 as c
    x = R.tone(c["f0"], c["n"], c["on"], c["off"], None, seed=1)
    lag, _peak, _nccf = _call(eng, [(x, x.size)], R.DEFAULT, nccf=False)
    R.check_tone(lag[0], R.DEFAULT, c["n"], c["on"], c["off"], None, R.SR / c["f0"])


def test_periods_and_noise_at_the_tiny_shape(eng):
    P = R.TINY
    rows = [(R.tiny_case(p), R.TINY_N) for p in R.TINY_PERIODS] + [(R.white(5, R.TINY_N), R.TINY_N)]
    lag, _peak, _nccf = _call(eng, rows, P)
    for b, p in enumerate(R.TINY_PERIODS):
        R.check_tone(lag[b], P, R.TINY_N, R.TINY_ON, R.TINY_OFF, None, p)
    assert (lag[5] == 0).all()


# ---- 4. the retime / pitch yardstick -------------------------------------------------------------------------------------------------------
def test_device_retime_then_device_pitch_stays_within_d_ref_plus_one(eng):
    """tests/test_pitch_cpu.py measures D_REF on the reference's own retiming; the device gets one more step of the lag grid, for score
    near-ties between neighbouring lags.  No voicing mismatch on the compared frames."""
    P = options.Pitch()
    RP = R.DEFAULT
    x = RT.voiced_signal(3, 48000)
    audio = torch.from_numpy(x).to(eng.device).view(1, 1, -1)
    lag_in = eng.pitch(audio, [x.size], P)[0].cpu().numpy()[0]
    for speed in R.YARD_SPEEDS:
        n_out = int(round(x.size / speed))
        out, lens = eng.retime(audio, [x.size], [np.asarray([[0, 0], [x.size, n_out]])], hop=240, delta=120)
        assert lens == [n_out]
        lag_out = eng.pitch(out.contiguous(), lens, P)[0].cpu().numpy()[0]
        d, unvoiced, pairs = R.yardstick(lag_in, lag_out, RP, x.size, n_out, speed)
        print(f"speed {speed}: {pairs} frames compared, worst deviation {d} lags, {unvoiced} unvoiced")
        assert unvoiced == 0 and pairs >= 150 and d <= R.D_REF + 1


# ---- 5. stability ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_two_calls_agree_rows_do_not_see_each_other_and_nccf_is_optional(eng, name):
    P = R.SHAPES[name]
    sig = _signals(name)
    rows = [(sig[0], sig[0].size - 5), (sig[1], sig[1].size // 2 + 3), (sig[3], sig[3].size)]
    lag, peak, nccf = _call(eng, rows, P)
    lag2, peak2, nccf2 = _call(eng, rows, P)
    assert np.array_equal(lag, lag2) and np.array_equal(_bits(peak), _bits(peak2)) and np.array_equal(_bits(nccf), _bits(nccf2))
    lag3, peak3, none = _call(eng, rows, P, nccf=False)
    assert none is None and np.array_equal(lag, lag3) and np.array_equal(_bits(peak), _bits(peak3))
    for b, (x, n) in enumerate(rows):
        l1, p1, s1 = _call(eng, [(x, n)], P, row_stride=sig[0].size)
        assert np.array_equal(lag[b], l1[0]) and np.array_equal(_bits(peak[b]), _bits(p1[0])) and np.array_equal(_bits(nccf[b]), _bits(s1[0])), b


# ---- 6. NaN ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "tiny"])
def test_nan_behind_len_changes_nothing(eng, name):
    P = R.SHAPES[name]
    sig = _signals(name)
    rows = [(sig[0], sig[0].size - P.reach - 7), (sig[1], sig[1].size // 2 + 3), (sig[3], 0)]
    clean = _call(eng, rows, P)
    dirty = _call(eng, rows, P, behind=np.nan)
    for a, b in zip(clean, dirty):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    assert not np.isnan(dirty[2][0, :P.frames(rows[0][1])]).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nan_or_inf_inside_len_stays_inside_its_windows_reach(eng, bad):
    P = R.DEFAULT
    x = R.tone(220.0, 24000, 1200, 22800, None, seed=6)
    at = 12345
    y = x.copy()
    y[at] = bad
    lag0, peak0, nccf0 = _call(eng, [(x, x.size)], P)
    lag, peak, nccf = _call(eng, [(y, y.size)], P)
    F = P.frames(x.size)
    assert (lag[0, :F] != LAG_SENTINEL).all() and (peak[0, :F] != SENTINEL).all() and (nccf[0, :F] != SENTINEL).all()   # all of it written
    s = np.arange(F) * P.hop
    touched = (s <= at) & (at < s + P.reach)
    assert touched.sum() >= 3 and np.array_equal(_bits(nccf[0, :F][~touched]), _bits(nccf0[0, :F][~touched]))
    assert np.isnan(nccf[0, :F][touched]).any() and not np.isinf(nccf[0, :F]).any()
    for f in np.flatnonzero(touched):                            # unvoiced, or voiced at a finite cost
        assert lag[0, f] == 0 or np.isfinite(nccf[0, f, lag[0, f] - P.lmin]), f
    assert np.array_equal(lag[0, :F][~touched], lag0[0, :F][~touched]) and np.array_equal(_bits(peak[0, :F][~touched]), _bits(peak0[0, :F][~touched]))
    _judge(f"one {bad}", P, [(y, y.size)], lag, peak, nccf, scores=False)


# ---- 7. guard bands -----------------------------------------------------------------------------------------------------------------------
def _arena(eng, d, P, B, tab=None):
    ar = Arena(eng.device)
    t = {k: ar.put(k, torch.from_numpy(d[k])) for k in ("audio", "len")}
    t["tab"] = ar.put("tab", torch.from_numpy(P.tab if tab is None else tab))
    t["lag"] = ar.alloc("lag", (B, d["Fmax"]), torch.int32)
    t["peak"] = ar.alloc("peak", (B, d["Fmax"], 3), torch.float32)
    t["nccf"] = ar.alloc("nccf", (B, d["Fmax"], P.L), torch.float32)
    t["ws"] = ar.workspace("ws", _ws_bytes(eng, B, d["S"], P))
    return ar, t


@pytest.mark.parametrize("name", sorted(R.SHAPES))
def test_guard_bands_stay_intact_and_do_not_matter(eng, name):
    P = R.SHAPES[name]
    sig = _signals(name)
    n = sig[0].size
    S = n - P.hop // 2 - 1                                       # a row_stride that is no multiple of hop: the last frame is partial
    rows = [(sig[0], 2 ** 40), (sig[1], -5), (sig[3], S - 3), (sig[0], n // 3)]      # len beyond row_stride, negative
    garbage = P.tab.copy()                                       # a table nobody checked
    garbage[0, ::7], garbage[1, 3::5], garbage[0, 1], garbage[1, 2] = np.nan, -3.0, np.inf, 1e30
    for tab, label in ((None, "the plan's table"), (garbage, "a table nobody checked")):
        d = _pack(rows, P, row_stride=S)
        ar, t = _arena(eng, d, P, len(rows), tab)
        got = []
        for with_nccf in (True, False):
            for byte in (0x00, 0xFF):
                ar.paint(byte)
                t["lag"].fill_(LAG_SENTINEL)                     # (paint() zeroed them: a stray write of 0 would hide)
                t["peak"].fill_(SENTINEL)
                t["nccf"].fill_(SENTINEL)
                t["ws"].fill_(byte ^ 0x5A)                       # what the workspace holds before the call does not matter
                assert _launch(eng, d, P, t, nccf=with_nccf) == 0, eng.lib.smtts_last_error(eng.h)
                ar.assert_clean("smtts_pitch", f"{name}, {label}, nccf {with_nccf} (guards 0x{byte:02X})")
                got.append((t["lag"].cpu().numpy().copy(), t["peak"].cpu().numpy().copy(), t["nccf"].cpu().numpy().copy()))
        for g in got[1:]:
            assert np.array_equal(got[0][0], g[0]) and np.array_equal(_bits(got[0][1]), _bits(g[1])), label
        assert np.array_equal(_bits(got[0][2]), _bits(got[1][2])) and (got[2][2] == SENTINEL).all() and (got[3][2] == SENTINEL).all()
        lag, peak, nccf = got[0]
        _judge(f"{name} {label}", P, rows, lag, peak, nccf, S=S, tab=tab, scores=tab is None)
        assert [_frames(P, x, ln, S) for x, ln in rows] == [d["Fmax"], 0, P.frames(S - 3), P.frames(n // 3)]


# ---- 8. refusals: one test each --------------------------------------------------------------------------------------------------------
_NAN, _INF = float("nan"), float("inf")
REFUSALS = ([{k: None} for k in ("audio", "len", "tab", "lag", "peak", "ws")]
            + [{"B": 0}, {"B": 1025}, {"row_stride": 0}, {"row_stride": 2 ** 24 + 1}, {"hop": 12}, {"hop": 1028}, {"hop": 18},
               {"win": 28}, {"win": 2052}, {"win": 66}, {"lmin": 1}, {"lmax": 8}, {"lmax": 7}, {"lmax": 2049}, {"lmin": 2, "lmax": 1025},
               {"bias": 0.0}, {"bias": -1.0}, {"bias": _NAN}, {"bias": _INF}]
            + [{k: v} for k in ("c_unv", "w_jump", "w_switch") for v in (-0.5, _NAN, _INF)]
            + [{"ws_bytes": "one short"}, {"ws": "not 256-byte aligned"}])
QUERY_REFUSALS = ((0, 64, 16, 8, 40), (1025, 64, 16, 8, 40), (1, 0, 16, 8, 40), (1, 2 ** 24 + 1, 16, 8, 40), (1, 64, 12, 8, 40),
                  (1, 64, 1028, 8, 40), (1, 64, 18, 8, 40), (1, 64, 16, 1, 40), (1, 64, 16, 40, 40), (1, 64, 16, 8, 2049), (1, 64, 16, 2, 1025))


def _case_id(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) if isinstance(o, dict) else "x".join(str(v) for v in o)


@pytest.fixture(scope="module")
def guarded_call(eng):
    """One good call's buffers between guards, shared by the refusal tests: (arena, tensors, host arrays)."""
    x = R.tiny_case(13)
    d = _pack([(x, x.size)], R.TINY)
    ar, t = _arena(eng, d, R.TINY, 1)
    return ar, t, d


def _nothing_was_enqueued(ar, t, what):
    torch.cuda.synchronize()
    ar.assert_clean("smtts_pitch", what)
    assert not t["lag"].any() and not t["peak"].any() and not t["nccf"].any() and not t["ws"].any(), what


@pytest.mark.parametrize("over", REFUSALS, ids=_case_id)
def test_a_refusal_names_the_entry_and_enqueues_nothing(eng, guarded_call, over):
    ar, t, d = guarded_call
    ar.paint(0xFF)                                               # ... and every output and the workspace are zero
    o = dict(over)
    if o.get("ws_bytes") == "one short":
        o["ws_bytes"] = int(t["ws"].numel()) - 1
    if o.get("ws") == "not 256-byte aligned":
        o["ws"] = C.c_void_p(t["ws"].data_ptr() + 128)
    assert _launch(eng, d, R.TINY, t, **o) == 1, over
    assert b"smtts_pitch: " in eng.lib.smtts_last_error(eng.h), (over, eng.lib.smtts_last_error(eng.h))
    _nothing_was_enqueued(ar, t, _case_id(over))


@pytest.mark.parametrize("bad", QUERY_REFUSALS, ids=_case_id)
def test_the_workspace_query_refuses_the_same_shapes(eng, bad):
    assert eng.lib.smtts_pitch_workspace_bytes(eng.h, *bad) == 0, bad
    assert b"smtts_pitch_workspace_bytes: " in eng.lib.smtts_last_error(eng.h), bad


def test_a_null_handle_is_refused_and_the_good_call_still_runs(eng, guarded_call):
    ar, t, d = guarded_call
    ar.paint(0xFF)
    lib = eng.lib
    assert lib.smtts_pitch(None, None, None, 1, 64, None, None, 16, 64, 8, 40, 1e-9, 0.5, 0.3, 0.3, None, None, None, None, 0) == 1
    assert b"smtts_pitch" in lib.smtts_last_error(None)
    assert lib.smtts_pitch_workspace_bytes(None, 1, 64, 16, 8, 40) == 0 and b"smtts_pitch_workspace_bytes" in lib.smtts_last_error(None)
    _nothing_was_enqueued(ar, t, "null handle")
    assert _launch(eng, d, R.TINY, t) == 0 and _launch(eng, d, R.TINY, t, nccf=False) == 0
    torch.cuda.synchronize()
    ar.assert_clean("smtts_pitch", "good")
    assert t["lag"].any() and t["nccf"].any()


# ---- 9. the public layers -------------------------------------------------------------------------------------------------------------------
def test_engine_pitch_is_the_entry(eng):
    P = R.DEFAULT
    sig = _signals("default")
    rows = [(sig[0], sig[0].size - 5), (sig[1], 0), (sig[3], 7001)]
    want_lag, want_peak, want_nccf = _call(eng, rows, P)
    audio = torch.from_numpy(_pack(rows, P)["audio"]).to(eng.device)
    lag, peak, nccf = eng.pitch(audio, [n for _x, n in rows], return_nccf=True)
    assert lag.dtype == torch.int32 and lag.shape == (3, 50) and peak.shape == (3, 50, 3) and nccf.shape == (3, 50, P.L)
    lag, peak, nccf = lag.cpu().numpy(), peak.cpu().numpy(), nccf.cpu().numpy()
    for b, (x, n) in enumerate(rows):
        F = P.frames(n)
        assert np.array_equal(lag[b, :F], want_lag[b, :F]) and np.array_equal(_bits(peak[b, :F]), _bits(want_peak[b, :F])), b
        assert np.array_equal(_bits(nccf[b, :F]), _bits(want_nccf[b, :F])) and not lag[b, F:].any() and not peak[b, F:].any() \
            and not nccf[b, F:].any(), b
    two = eng.pitch(audio, [n for _x, n in rows], options.Pitch())
    assert len(two) == 2 and np.array_equal(two[0].cpu().numpy(), lag)
    tiny = eng.pitch(audio[:, :, :1600].contiguous(), [1600, 0, 800], options.Pitch(fmin=600, fmax=3000, hop=16, win=64))
    assert tiny[0].shape == (3, 100) and tiny[1].shape == (3, 100, 3)
    with pytest.raises(ValueError, match="pitch: "):
        eng.pitch(audio, [1, 2])


@pytest.fixture(scope="module")
def tts(eng):
    from smalltts_amd.api import SmallTTS
    return SmallTTS(engine=eng, seed=0)


def test_thirty_one_seconds_take_two_rows_that_agree_with_one(eng, tts):
    from smalltts_amd import api
    n = 31 * 24000
    x = R.tone(150.0, n, 2400, n - 2400, (400000, 402400), seed=8)
    rows = plans.pitch_rows(n, 240)
    assert len(rows) == 2
    track = tts.pitch(x)
    assert isinstance(track, api.PitchTrack) and track.hop == 240 and track.sr == 24000 and track.f0.shape == (3100,) == track.strength.shape
    lag1, peak1 = eng.pitch(torch.from_numpy(x).to(eng.device).view(1, 1, -1), [n])              # the same as ONE row
    f1, s1 = plans.pitch_f0(lag1.cpu().numpy()[0], peak1.cpu().numpy()[0])
    f = np.arange(3100)
    shared = (f * 240 >= rows[1][0]) & (f * 240 < rows[0][0] + rows[0][1])
    assert shared.sum() == 100 and rows[1][2] == rows[1][0] // 240 + 50
    assert np.array_equal(track.f0[~shared], f1[~shared]) and np.array_equal(_bits(track.strength[~shared]), _bits(s1[~shared]))
    both = (track.f0 > 0) & (f1 > 0)
    assert np.array_equal(track.f0 > 0, f1 > 0) and (np.abs(24000 / track.f0[both & shared] - 24000 / f1[both & shared]) <= 1.0 + 1e-9).all()
    inner = R.inside(R.DEFAULT, n, [(2400, 400000), (402400, n - 2400)])
    assert (np.abs(track.f0[inner] - 150.0) <= 150.0 ** 2 / 24000).all()
    # word statistics
    words = [(0, "word", "a", 24000, 48000, -0.1), (1, "punct", ",", 48000, 48000, -0.1), (2, "word", "b", 0, 1200, -0.2),
             (3, "word", "c", 399000, 402400, -0.3)]
    track2, stats = tts.pitch(x, words=words)
    assert np.array_equal(track2.f0, track.f0) and [w for w, _s in stats] == words
    st = [s for _w, s in stats]
    assert st == plans.pitch_word_stats(words, track.f0, 240)
    assert abs(st[0]["f0_median"] - 150.0) < 1.0 and st[0]["voiced"] == 1.0 and st[1]["f0_median"] is None and st[2]["voiced"] == 0.0
    assert 0.0 < st[3]["voiced"] < 0.6                             # the hole takes most of the word
    with pytest.raises(ValueError, match="pitch: "):
        tts.pitch(np.zeros((2, 5), np.float32))
    with pytest.raises(TypeError, match="pitch must be"):
        tts.pitch(x, pitch=0.5)
    # several rows in one call: rows of 2 s against the one row
    y = torch.from_numpy(x[:96000]).to(eng.device)
    a = api._pitch_device(eng, y, options.Pitch(), max_row=48000)
    b = api._pitch_device(eng, y, options.Pitch())
    assert len(plans.pitch_rows(96000, 240, max_row=48000)) == 3 and a[0].shape == b[0].shape == (400,)
    assert np.array_equal(a[0] > 0, b[0] > 0) and np.abs(a[0] - b[0]).max() <= 1


def test_pitch_wav_resamples_first_and_the_command_line_writes_the_track(eng, tts, tmp_path):
    from smalltts_amd.audio import write_wav_pcm16
    from smalltts_amd.scripts import pitch as cli
    from smalltts_amd.scripts.align import words_json
    sr = 16000
    x = R.tone(220.0, sr, 1600, 14400, None, seed=9, floor=1e-4, sr=sr)                     # 1 s at 16 kHz
    track = tts.pitch_wav(x, sr)
    assert track.sr == 24000 and track.hop == 240 and track.f0.shape == (100,)
    inner = R.inside(R.DEFAULT, 24000, [(2400 + 200, 21600 - 200)])                         # (the resampler's own reach left out)
    assert inner.sum() >= 30 and (np.abs(track.f0[inner] - 220.0) <= 220.0 ** 2 / 24000).all() and (track.f0[:5] == 0).all()
    wav, words_in, out, csv = tmp_path / "in.wav", tmp_path / "w.json", tmp_path / "o" / "f0.json", tmp_path / "o" / "f0.csv"
    write_wav_pcm16(str(wav), x, sr)
    words = [(0, "word", "ab", 6000, 18000, -0.5), (1, "punct", ",", 18000, 18000, float("-inf"))]
    words_in.write_text(words_json(words), encoding="utf-8")
    cli.main(["--wav", str(wav), "--words", str(words_in), "--out", str(out), "--csv", str(csv)])
    doc = json.loads(out.read_text(encoding="utf-8"))
    assert doc["hop"] == 240 and doc["sr"] == 24000 and len(doc["f0"]) == 100 == len(doc["strength"])
    got = np.asarray(doc["f0"])
    assert (np.abs(got[inner] - 220.0) <= 220.0 ** 2 / 24000).all()                                       # (PCM16 in between)
    assert abs(doc["words"][0]["f0_median"] - 220.0) < 220.0 ** 2 / 24000 and doc["words"][0]["voiced"] == 1.0
    assert doc["words"][1]["f0_median"] is None and doc["words"][0]["start"] == 6000
    lines = csv.read_text(encoding="utf-8").splitlines()
    assert len(lines) == 100 and lines[1].startswith("0.0100,")
    cli.main(["--wav", str(wav), "--out", str(out), "--fmin", "100", "--fmax", "300"])
    assert "words" not in json.loads(out.read_text(encoding="utf-8"))
