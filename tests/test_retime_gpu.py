"""GPU: retiming (include/smalltts_hip.h smtts_retime).  The kernel against the numpy restatement of
tests/helpers/retime_ref.py: teacher-forced on every case (each segment judged given the device's own previous choice, at the
derived bound of an fp32 dot product, and exactly where the float64 argmax is clear; the overlap-add driven by the device's q BIT FOR
BIT), free-running and exact on the cases tests/test_retime_cpu.py shows to be clear; identity, row independence, determinism,
nothing behind len, guard bands, refusals; and the public layers on top (HipEngine.retime, SmallTTS.retime, synthesize_long(retime=))
on the small engine of the API tests.  No tolerance here is a tuned number."""
import ctypes as C

import numpy as np
import pytest
import torch

from smalltts_amd import plans
from tests.helpers import retime_ref as R
from tests.helpers import watermark_ref as W
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
SENTINEL, Q_SENTINEL = 7.25, -77


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


def _pack(rows, hop, A=None, out_stride=None, row_stride=None, n_anchor=None, behind=0.0):
    """Rows (dicts of x, len, anchors) -> the host arrays of one call: audio (B,1,S) (`behind` behind every len), len, anchors
    (B,A,2) zero-padded, n_anchor, and out_stride / Kmax."""
    B = len(rows)
    S = max(r["x"].size for r in rows) if row_stride is None else row_stride
    A = max(len(r["anchors"]) for r in rows) if A is None else A
    audio = np.full((B, 1, S), behind, np.float32)
    anc = np.zeros((B, A, 2), np.int64)
    for b, r in enumerate(rows):
        n = max(0, min(int(r["len"]), r["x"].size))
        audio[b, 0, :n] = r["x"][:n]
        anc[b, :len(r["anchors"])] = r["anchors"]
    ln = np.asarray([r["len"] for r in rows], np.int64)
    na = np.asarray([len(r["anchors"]) for r in rows] if n_anchor is None else n_anchor, np.int64)
    out_stride = max(int(r["anchors"][-1][1]) for r in rows) if out_stride is None else out_stride
    return dict(audio=audio, len=ln, anchors=anc, n_anchor=na, A=A, S=S, out_stride=out_stride, Kmax=-(-out_stride // hop), hop=hop)


def _launch(eng, d, delta, t, want_q=True):
    """smtts_retime on device tensors t (audio, len, anchors, n_anchor, win, out, q)."""
    return eng.lib.smtts_retime(eng.h, eng._stream(), _p(t["audio"]), d["audio"].shape[0], d["S"], _p(t["len"]), _p(t["anchors"]),
                                _p(t["n_anchor"]), d["A"], _p(t["win"]), d["hop"], delta, _p(t["out"]), d["out_stride"],
                                _p(t["q"]) if want_q else None)


def _call(eng, rows, hop, delta, **kw):
    """One call on plain tensors -> (out (B, out_stride) filled with SENTINEL first, q (B, Kmax) filled with Q_SENTINEL first)."""
    d = _pack(rows, hop, **kw)
    t = {k: torch.from_numpy(d[k]).to(eng.device) for k in ("audio", "len", "anchors", "n_anchor")}
    t["win"] = torch.from_numpy(R.window(hop)).to(eng.device)
    t["out"] = torch.full((len(rows), 1, d["out_stride"]), SENTINEL, device=eng.device)
    t["q"] = torch.full((len(rows), d["Kmax"]), Q_SENTINEL, dtype=torch.int64, device=eng.device)
    assert _launch(eng, d, delta, t) == 0, eng.lib.smtts_last_error(eng.h)
    return t["out"].cpu().numpy()[:, 0], t["q"].cpu().numpy(), d


def _judge(name, row, out, q, d, hop, delta):
    """The teacher-forced check of one row of a call -> (the reference's result driven by the device's q, searched, clear)."""
    m, table = len(row["anchors"]), row["anchors"]
    probe = R.retime_row(row["x"], row["len"], table, m, R.window(hop), hop, delta, d["out_stride"], row_stride=d["S"])
    K, out_len = probe["K"], probe["out_len"]
    assert (q[K:] == Q_SENTINEL).all() and (out[out_len:] == SENTINEL).all(), name     # nothing at or behind K / out_len
    qd = q[:K]
    ref = R.retime_row(row["x"], row["len"], table, m, R.window(hop), hop, delta, d["out_stride"], q_forced=qd, row_stride=d["S"])
    n_clear = n_search = 0
    for k in range(K):
        seg = ref["segments"][k]
        if k == 0:
            assert qd[0] == ref["p"][0], name
        elif seg is None:
            assert qd[k] == qd[k - 1] + hop, (name, k)                                   # the continuation rule
        else:
            n_search += 1
            lag = int(qd[k] - seg["p"])
            assert lag in seg["lags"], (name, k, lag)
            i, b = seg["lags"].index(lag), seg["best"]
            assert seg["score"][i] >= seg["score"][b] - seg["E"][i] - seg["E"][b], (name, k, lag, seg["lags"][b])
            if R.is_clear(dict(segments=[seg])):
                n_clear += 1
                assert i == b, (name, k, lag, seg["lags"][b])
    assert np.array_equal(_bits(out[:out_len]), _bits(ref["out"])), name                 # three fp32 operations: bit for bit
    return ref, n_search, n_clear


# ---- 1. teacher-forced: every case ---------------------------------------------------------------------------------------------------
CASES = R.teacher_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_segment_is_right_given_the_devices_own_previous_choice(eng, name):
    c = CASES[name]
    out, q, d = _call(eng, [c], c["hop"], c["delta"])
    ref, n_search, n_clear = _judge(name, c, out[0], q[0], d, c["hop"], c["delta"])
    print(f"{name}: {ref['K']} segments, {n_search} searched, {n_clear} of them clear")
    if "speed" in name or name.startswith(("wordlike", "burst", "partial")):
        assert n_search >= 10, (name, n_search)


# ---- 2. free-running equality on the clear cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.clear_cases()))
def test_the_clear_cases_equal_the_free_reference_exactly(eng, name):
    c = R.clear_cases()[name]
    out, q, d = _call(eng, [c], c["hop"], c["delta"])
    ref = R.retime_row(c["x"], c["len"], c["anchors"], 2, R.window(c["hop"]), c["hop"], c["delta"], d["out_stride"])
    assert R.searched(ref) >= 10
    assert np.array_equal(q[0, :ref["K"]], ref["q"]) and np.array_equal(_bits(out[0, :ref["out_len"]]), _bits(ref["out"]))


# ---- 3. identity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,delta", R.SHAPES)
def test_a_unit_map_returns_the_inputs_bits(eng, hop, delta):
    n = 50 * hop + 7
    for name in sorted(R.SIGNALS):
        x = R.SIGNALS[name](3, n)
        out, q, d = _call(eng, [dict(x=x, len=n, anchors=np.asarray([[0, 0], [n, n]]))], hop, delta)
        assert np.array_equal(_bits(out[0]), _bits(x)) and (q[0] == np.arange(d["Kmax"]) * hop).all()


# ---- 4. rows are independent, 5. determinism, 6. nothing behind len matters ----------------------------------------------------------
def _three_rows(hop):
    a = R.uniform_case("voiced", hop, 0, 0.8)
    b = dict(x=R.noise_signal(31, 33 * hop + 5), len=33 * hop + 5, anchors=R.wordlike_anchors(hop)[:8])
    c = dict(x=R.voiced_signal(32, 20 * hop), len=17 * hop + 3, anchors=np.asarray([[0, 0], [17 * hop + 3, 11 * hop + 9]], np.int64))
    return [a, b, c]


@pytest.mark.parametrize("hop,delta", R.SHAPES)
def test_rows_do_not_see_each_other_and_two_calls_agree(eng, hop, delta):
    rows = _three_rows(hop)
    out, q, d = _call(eng, rows, hop, delta)
    out2, q2, _d = _call(eng, rows, hop, delta)
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(q, q2)            # two calls, equal bits
    for b, r in enumerate(rows):
        one, q1, d1 = _call(eng, [r], hop, delta)
        n, K = int(r["anchors"][-1][1]), -(-int(r["anchors"][-1][1]) // hop)
        assert np.array_equal(_bits(out[b, :n]), _bits(one[0, :n])) and np.array_equal(q[b, :K], q1[0, :K]), b
        assert (out[b, n:] == SENTINEL).all() and (q[b, K:] == Q_SENTINEL).all(), b
        _judge(f"row {b}", r, one[0], q1[0], d1, hop, delta)


@pytest.mark.parametrize("hop,delta", R.SHAPES)
def test_nan_behind_len_reaches_nothing(eng, hop, delta):
    rows = _three_rows(hop)
    S = max(r["x"].size for r in rows) + 2 * hop + delta + 3                             # room behind every row, all of it NaN
    clean, qc, _d = _call(eng, rows, hop, delta, row_stride=S)
    dirty, qd, _d = _call(eng, rows, hop, delta, row_stride=S, behind=np.nan)
    for b, r in enumerate(rows):
        n = int(r["anchors"][-1][1])
        assert not np.isnan(dirty[b, :n]).any(), b
    assert np.array_equal(_bits(clean), _bits(dirty)) and np.array_equal(qc, qd)


def test_a_nan_score_counts_as_minus_infinity(eng):
    """NaN samples INSIDE len: every score that touches them is NaN and, by the header, -inf.  A row that is NaN throughout has only
    such scores, so the tie rule decides every searched segment: lag 0.  A row with one NaN sample: the candidates that avoid it win
    over those that do not, and the reference (which applies the same rule in float64) is followed bit for bit where it is driven by
    the device's q."""
    hop, delta = 32, 8
    n = 40 * hop
    table = np.asarray([[0, 0], [n, int(n / 1.6)]], np.int64)
    allnan = dict(x=np.full((n,), np.nan, np.float32), len=n, anchors=table)
    one = R.noise_signal(61, n)
    one[17 * hop + 5] = np.nan
    out, q, d = _call(eng, [allnan, dict(x=one, len=n, anchors=table)], hop, delta)
    out2, q2, _d = _call(eng, [allnan, dict(x=one, len=n, anchors=table)], hop, delta)
    assert np.array_equal(_bits(out), _bits(out2)) and np.array_equal(q, q2)
    K = -(-int(table[-1, 1]) // hop)
    ref = R.retime_row(allnan["x"], n, table, 2, R.window(hop), hop, delta, d["out_stride"], q_forced=q[0, :K])
    searched = [k for k in range(K) if ref["segments"][k] is not None]
    assert len(searched) >= 10 and all(q[0, k] == ref["p"][k] for k in searched)
    ref = R.retime_row(one, n, table, 2, R.window(hop), hop, delta, d["out_stride"], q_forced=q[1, :K])
    got, want = out[1, :ref["out_len"]], ref["out"]              # (a NaN's payload is the platform's: compared as "NaN here too")
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any()
    assert np.array_equal(_bits(got[~np.isnan(want)]), _bits(want[~np.isnan(want)]))
    mixed = 0
    for k in range(1, K):
        seg = ref["segments"][k]
        if seg is None:
            assert q[1, k] == q[1, k - 1] + hop
            continue
        i = seg["lags"].index(int(q[1, k] - seg["p"]))
        fin = np.isfinite(seg["score"])
        if fin.any():
            assert fin[i], (k, seg["lags"][i])                   # a NaN score never beats a number
            mixed += (~fin).any()
        else:
            assert seg["lags"][i] == 0, k
    assert mixed >= 1


# ---- 7. bounds ------------------------------------------------------------------------------------------------------------------------
def _garbage_rows(hop):
    """Tables a host check would refuse: anchors that do not increase, that run backwards, beyond both strides, below zero; with
    n_anchor larger than A, negative, and 1."""
    x = R.voiced_signal(41, 30 * hop)
    big = 2 ** 62
    tabs = [[[0, 0], [5 * hop, 4 * hop], [5 * hop, 4 * hop], [3 * hop, 9 * hop], [20 * hop, 7 * hop], [30 * hop, 25 * hop + 3]],
            [[7, 3 * hop], [-big, hop], [big, 2 * hop], [hop, 2 * hop], [12 * hop, 30 * hop], [big, big]],
            [[0, 0], [10 * hop, 10 * hop], [0, 0], [0, 0], [0, 0], [0, 0]],
            [[0, 0], [10 * hop, 10 * hop], [0, 0], [0, 0], [0, 0], [0, 0]],
            [[0, 0], [10 * hop, 10 * hop], [0, 0], [0, 0], [0, 0], [0, 0]]]
    lens = [30 * hop, 30 * hop - 1, 2 ** 40, -5, 30 * hop]
    return [dict(x=x, len=n, anchors=np.asarray(t, np.int64)) for t, n in zip(tabs, lens)], [6, 2 ** 40, 2, 2, 1]


@pytest.mark.parametrize("hop,delta", R.SHAPES)
def test_guard_bands_stay_intact_and_do_not_matter(eng, hop, delta):
    good = _three_rows(hop)
    bad, bad_m = _garbage_rows(hop)
    for rows, kw, label in ((good, {}, "valid tables"),
                            (bad, dict(n_anchor=bad_m, out_stride=26 * hop + 1, row_stride=30 * hop), "tables nobody checked")):
        d = _pack(rows, hop, **kw)
        ar = Arena(eng.device)
        t = {k: ar.put(k, torch.from_numpy(d[k])) for k in ("audio", "len", "anchors", "n_anchor")}
        t["win"] = ar.put("win", torch.from_numpy(R.window(hop)))
        t["out"] = ar.alloc("out", (len(rows), 1, d["out_stride"]), torch.float32)
        t["q"] = ar.alloc("q", (len(rows), d["Kmax"]), torch.int64)
        got = []
        for byte in (0x00, 0xFF):
            ar.paint(byte)
            t["out"].fill_(SENTINEL)                             # (paint() zeroed them: a stray write of 0.0 or of q = 0 would hide)
            t["q"].fill_(Q_SENTINEL)
            assert _launch(eng, d, delta, t) == 0, eng.lib.smtts_last_error(eng.h)
            ar.assert_clean("smtts_retime", f"{label} {hop}x{delta} (guards 0x{byte:02X})")
            got.append((t["out"].cpu().numpy()[:, 0].copy(), t["q"].cpu().numpy().copy()))
        assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(got[0][1], got[1][1]), label
        out, q = got[0]
        for b, r in enumerate(rows):                             # ... and the result is the contract's, whatever the table holds
            m = kw["n_anchor"][b] if "n_anchor" in kw else len(r["anchors"])
            probe = R.retime_row(r["x"], r["len"], d["anchors"][b], m, R.window(hop), hop, delta, d["out_stride"], row_stride=d["S"])
            K, n = probe["K"], probe["out_len"]
            assert (out[b, n:] == SENTINEL).all() and (q[b, K:] == Q_SENTINEL).all(), (label, b)   # nobody wrote there
            ref = R.retime_row(r["x"], r["len"], d["anchors"][b], m, R.window(hop), hop, delta, d["out_stride"], q_forced=q[b, :K],
                               row_stride=d["S"])
            assert np.array_equal(_bits(out[b, :n]), _bits(ref["out"])), (label, b)
            for k in range(K):
                seg = ref["segments"][k]
                if k and seg is None:
                    assert q[b, k] == q[b, k - 1] + hop, (label, b, k)
                elif k:
                    assert int(q[b, k] - seg["p"]) in seg["lags"], (label, b, k)
                else:
                    assert q[b, 0] == ref["p"][0], (label, b)
        if rows is bad:
            assert [R.retime_row(r["x"], r["len"], d["anchors"][b], bad_m[b], R.window(hop), hop, delta, d["out_stride"],
                                 row_stride=d["S"])["out_len"] for b, r in enumerate(rows)] == [25 * hop + 3, 26 * hop + 1, 10 * hop,
                                                                                              10 * hop, 0]


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_entry_and_enqueue_nothing(eng):
    hop, delta = 32, 8
    c = R.uniform_case("noise", hop, delta, 1.25)
    d = _pack([c], hop)
    ar = Arena(eng.device)
    t = {k: ar.put(k, torch.from_numpy(d[k])) for k in ("audio", "len", "anchors", "n_anchor")}
    t["win"] = ar.put("win", torch.from_numpy(R.window(hop)))
    t["out"] = ar.alloc("out", (1, 1, d["out_stride"]), torch.float32)
    t["q"] = ar.alloc("q", (1, d["Kmax"]), torch.int64)
    ar.paint(0xFF)
    lib = eng.lib

    def call(**over):
        a = dict(audio=_p(t["audio"]), B=1, row_stride=d["S"], len=_p(t["len"]), anchors=_p(t["anchors"]), n_anchor=_p(t["n_anchor"]),
                 A=d["A"], win=_p(t["win"]), hop=hop, delta=delta, out=_p(t["out"]), out_stride=d["out_stride"], q=_p(t["q"]))
        a.update(over)
        return lib.smtts_retime(eng.h, eng._stream(), a["audio"], a["B"], a["row_stride"], a["len"], a["anchors"], a["n_anchor"], a["A"],
                                a["win"], a["hop"], a["delta"], a["out"], a["out_stride"], a["q"])

    for over in ([{k: None} for k in ("audio", "len", "anchors", "n_anchor", "win", "out")]
                 + [{"B": 0}, {"B": 1025}, {"row_stride": 0}, {"row_stride": 2 ** 31}, {"out_stride": 0}, {"out_stride": 2 ** 31},
                    {"A": 1}, {"A": 65537}, {"hop": 12}, {"hop": 516}, {"hop": 34}, {"delta": -1}, {"delta": 513}]):
        assert call(**over) == 1, over
        assert b"smtts_retime" in lib.smtts_last_error(eng.h), (over, lib.smtts_last_error(eng.h))
    assert lib.smtts_retime(None, None, None, 1, 1, None, None, None, 2, None, 32, 8, None, 1, None) == 1
    assert b"smtts_retime" in lib.smtts_last_error(None)
    torch.cuda.synchronize()
    ar.assert_clean("smtts_retime", "refusals")
    assert not t["out"].any() and not t["q"].any()                                   # nothing was enqueued
    assert call() == 0 and call(q=None) == 0
    torch.cuda.synchronize()
    ar.assert_clean("smtts_retime", "good")
    assert t["out"].any()


# ---- the engine's method -------------------------------------------------------------------------------------------------------------
def test_engine_retime_is_the_entry(eng):
    hop, delta = 240, 120
    rows = _three_rows(hop)
    want, wq, d = _call(eng, rows, hop, delta)
    audio = torch.from_numpy(d["audio"]).to(eng.device)
    out, lens, q = eng.retime(audio, [r["len"] for r in rows], [r["anchors"] for r in rows], return_q=True)
    assert lens == [int(r["anchors"][-1][1]) for r in rows] and out.shape == (3, 1, max(lens)) and q.shape == wq.shape
    out, q = out.cpu().numpy()[:, 0], q.cpu().numpy()
    for b, n in enumerate(lens):
        K = -(-n // hop)
        assert np.array_equal(_bits(out[b, :n]), _bits(want[b, :n])) and (out[b, n:] == 0).all(), b
        assert np.array_equal(q[b, :K], wq[b, :K]) and (q[b, K:] == 0).all(), b
    with pytest.raises(ValueError, match="retime: "):
        eng.retime(audio, [r["len"] for r in rows], [r["anchors"] for r in rows[:2]])


# ---- 9. through the API ---------------------------------------------------------------------------------------------------------------
REF = torch.randn(5, 64, generator=torch.Generator().manual_seed(0)).numpy()
TOKS = [3, 17, 42, 99, 150, 7, 8]


@pytest.fixture(scope="module")
def tts(eng):
    from smalltts_amd.api import SmallTTS
    return SmallTTS(engine=eng, seed=0)


def test_synthesize_long_retimes_the_joined_waveform(eng, tts):
    from smalltts_amd.api import Delivery, Retime
    voice = tts.encode_voice(REF)
    kw = dict(token_lists=[TOKS, TOKS[:4], TOKS[2:]], durations=[0.8, 0.3, 0.5], seed=3, max_batch=2)
    plain, segs, words = tts.synthesize_long(voice, return_segments=True, return_words=True, **kw)
    assert np.array_equal(tts.synthesize_long(voice, retime=None, **kw).view(np.uint32), plain.view(np.uint32))
    same, s1, w1 = tts.synthesize_long(voice, retime=Retime(speed=1.0), return_segments=True, return_words=True, **kw)
    assert same.dtype == plain.dtype and np.array_equal(same.view(np.uint32), plain.view(np.uint32)) and (s1, w1) == (segs, words)
    S = plain.shape[1]
    dur = 1.3171
    got, gsegs, gwords = tts.synthesize_long(voice, retime=Retime(duration=dur), return_segments=True, return_words=True, **kw)
    n = int(round(dur * 24000))
    assert got.shape == (1, n) and got.dtype == np.float32 and n != S and np.abs(got).max() > 0
    table = np.asarray([[0, 0], [S, n]])
    assert gsegs == [(plans.retime_times(o, table), plans.retime_times(o + m, table) - plans.retime_times(o, table), st, g)
                     for o, m, st, g in segs]
    assert gwords == [(i, kind, plans.retime_times(a, table), plans.retime_times(b, table)) for i, kind, a, b in words]
    ends = [v for o, m, _st, _g in gsegs for v in (o, o + m)]
    assert ends == sorted(ends) and ends[0] >= 0 and ends[-1] <= n                       # inside the output, monotone
    wends = [v for _i, _k, a, b in gwords for v in (a, b)]
    assert all(0 <= a <= b <= n for _i, _k, a, b in gwords) and [w[2] for w in gwords] == sorted(w[2] for w in gwords), wends
    # the device's waveform is engine.retime of the plain call's
    want, lens = eng.retime(torch.from_numpy(plain[None]).to(eng.device), [S], [table])
    assert np.array_equal(got.view(np.uint32), want[0, :, :n].cpu().numpy().view(np.uint32))
    # behind the retiming: the delivery has the length of the retimed length, a number is a speed
    dv = Delivery(16000, "mulaw")
    d = tts.synthesize_long(voice, retime=Retime(duration=dur), deliver=(16000, "mulaw"), **kw)
    assert d.dtype == dv.dtype and d.shape == (1, dv.samples(n))
    fast = tts.synthesize_long(voice, retime=1.25, **kw)
    assert fast.shape == (1, int(round(S / 1.25)))
    # render_long shares the tail
    _w, pieces = tts.synthesize_long(voice, return_pieces=True, **kw)
    again = tts.render_long(pieces, max_batch=2, retime=Retime(duration=dur))
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    for bad, match in ((dict(retime=Retime(to_words=[(0, "word", "x", 0, 5, 0.0)])), "SmallTTS.retime"),
                       (dict(retime=Retime(speed=1.1), pcm16=True), "pcm16")):
        with pytest.raises(ValueError, match=match):
            tts.synthesize_long(voice, **kw, **bad)
    with pytest.raises(ValueError, match="retime"):
        tts.synthesize_long_stream(voice, retime=1.1, **kw)


def test_a_mark_is_embedded_in_the_samples_that_leave(eng, tts):
    from smalltts_amd.api import Retime
    voice = tts.encode_voice(REF)
    kw = dict(token_lists=[TOKS, TOKS[2:]], durations=[0.8, 0.5], seed=3)
    got = tts.synthesize_long(voice, retime=Retime(speed=0.9), watermark=(1234, 0.05), **kw)
    bare = tts.synthesize_long(voice, retime=Retime(speed=0.9), **kw)
    plain = tts.synthesize_long(voice, **kw)
    assert bare.shape == (1, int(round(plain.shape[1] / 0.9)))
    assert got.shape == bare.shape and np.array_equal(_bits(got[0]), _bits(W.embed(bare[0], 1234, 0.05)))


# ---- 10. words land where they were sent -----------------------------------------------------------------------------------------------
def test_words_land_where_they_were_sent(eng, tts):
    from smalltts_amd.api import Retime
    n = 60000
    x = R.voiced_signal(51, n)
    now = [(0, "word", "a", 2000, 9000, -0.1), (1, "punct", ",", 9000, 9000, -0.1), (2, "word", "b", 14000, 22000, -0.2),
           (3, "word", "c", 22500, 24000, -0.1), (4, "word", "d", 40000, 52000, -0.3)]
    to = [(0, "word", "a", 3000, 8000, 0.0), (1, "punct", ",", 0, 0, 0.0), (2, "word", "b", 12000, 24000, 0.0),
          (3, "word", "c", 24100, 24300, 0.0), (4, "word", "d", 30000, 41000, 0.0)]
    out, mapped, clamped = tts.retime(x, Retime(to_words=to), words=now)
    assert clamped == [3] and out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == 1
    for w, m, t in zip(now, mapped, to):
        assert m[:3] == w[:3] and m[5] == w[5]
        if w[1] == "word" and w[0] not in clamped:
            assert (m[3], m[4]) == (t[3], t[4]), (w, m, t)
    assert mapped[3][3] == 24100 and mapped[3][4] == 24100 + 750                          # 1500 samples at max_rate 2
    assert out.shape[1] == mapped[4][4] + (n - 52000) and np.abs(out).max() <= 1.0
    # a uniform speed through the same door, and a long input through the rows
    fast, none, clamped = tts.retime(x, 1.25)
    assert fast.shape == (1, 48000) and none is None and clamped == []
    anchors, _c = plans.retime_anchors(n, words=now, to_words=to)
    y = torch.from_numpy(x).to(eng.device)
    joined, table = tts._retime_device(y, anchors, now, Retime(to_words=to), max_row=24000)
    rows, table2 = plans.retime_rows(n, anchors, now, max_row=24000)
    assert len(rows) > 2 and np.array_equal(table, table2) and joined.numel() == int(table[-1, 1])
    parts = [eng.retime(y[s0: s0 + sn].reshape(1, 1, -1).contiguous(), [sn], [tab])[0].view(-1) for s0, sn, _d0, tab in rows]
    assert np.array_equal(joined.cpu().numpy().view(np.uint32), torch.cat(parts).cpu().numpy().view(np.uint32))
