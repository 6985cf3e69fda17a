"""GPU: the watermark (include/smalltts_hip.h smtts_watermark, smtts_watermark_detect).  The embedder against the float32
restatement of tests/helpers/watermark_ref.py BIT FOR BIT, whole and chunked, with the carried slot checked after every call; the
detector's u against the fp64 restatement at the bound counted next to it, T and den against fp64 sums of the device's own u at the
bound the stated summation order gives, best_off and best_z exactly; guard bands and refusals; and the public layers on top
(synthesize_stream, synthesize_long, synthesize_long_stream, DecodeStream, detect_watermark) on the small engine of the API tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import deliver_ref as DR
from tests.helpers import watermark_ref as W
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
KEY = 0x5EEDC0DE12345678
STRENGTH = 0.02
S = 1024
LENS = (1, 64, 200, 1000)
CHUNKS = (1, 63, 64, 65, 127, 128, 300)          # ... then the rest
SLOTS = (2, 0, 3, 1)                              # a non-identity slot table; slot 4 of the pool belongs to nobody


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


def _signal(B, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.3 * np.sin(0.05 * t)[None] * (1 + 0.5 * np.sin(0.003 * t + np.arange(B)[:, None])) + 0.02 * rng.standard_normal((B, n))
    return x.astype(np.float32)


def _embed(eng, audio, table, pool, n_slots, out, key=KEY, strength=STRENGTH, B=None, row=None):
    B = int(audio.shape[0]) if B is None else B
    row = int(audio.shape[-1]) if row is None else row
    return eng.lib.smtts_watermark(eng.h, eng._stream(), _p(audio), B, row, _p(table), key, strength, _p(pool), n_slots, _p(out))


def _table(eng, rows):
    return torch.tensor(rows, dtype=torch.int64, device=eng.device)


SENTINEL = 7.25


# ---- 1. the embedder against the restatement, bit for bit ------------------------------------------------------------------------------
def test_whole_embedding_is_the_restatement_bit_for_bit(eng):
    x = _signal(4, S, 1)
    audio = torch.from_numpy(x[:, None]).to(eng.device)
    tab = _table(eng, [[9, 123, n, 0] for n in LENS])          # no pool: slot and n_before are ignored
    outs = []
    for _run in range(2):
        out = torch.full_like(audio, SENTINEL)
        assert _embed(eng, audio, tab, None, 0, out) == 0, eng.lib.smtts_last_error(eng.h)
        outs.append(out.cpu().numpy()[:, 0])
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))       # two runs, equal bits
    for b, n in enumerate(LENS):
        assert np.array_equal(_bits(outs[0][b, :n]), _bits(W.embed(x[b, :n], KEY, STRENGTH))), b
        assert (outs[0][b, n:] == SENTINEL).all(), b            # nothing is written behind len
    assert not np.array_equal(outs[0][3, 64:1000], x[3, 64:1000])
    # the wrapper: the same, and strength 0 changes no value
    got = eng.watermark(audio, LENS, KEY, STRENGTH).cpu().numpy()[:, 0]
    assert all(np.array_equal(_bits(got[b, :n]), _bits(outs[0][b, :n])) for b, n in enumerate(LENS))
    assert np.array_equal(eng.watermark(audio, LENS, KEY, 0.0).cpu().numpy()[3, 0, :1000], x[3, :1000])


@pytest.mark.parametrize("start", [0, 2 ** 33 + 5, 2 ** 39 + 5])
def test_chunked_embedding_is_whole_embedding_bit_for_bit(eng, start):
    """Four streams of LENS samples through one pool in chunks of CHUNKS, then the rest; a stream that has ended passes len 0.
    start = 2^33 + 5: positions past 32 bits; 2^39 + 5: the Philox counter's high word is 1."""
    x = _signal(4, S, 2)
    refs = [W.Stream(KEY, STRENGTH, start=start) for _ in LENS]
    pool = torch.zeros(5, 128, device=eng.device)
    pool[4] = SENTINEL
    assert pool.element_size() * 128 == eng.lib.smtts_watermark_state_bytes(eng.h) == 512
    done = [0] * 4
    got = [[] for _ in LENS]
    sizes = list(CHUNKS) + [S]
    for c in sizes:
        ln = [min(c, n - d) for n, d in zip(LENS, done)]
        audio = torch.full((4, 1, S), np.nan, device=eng.device)
        for b in range(4):
            audio[b, 0, :ln[b]] = torch.from_numpy(x[b, done[b]: done[b] + ln[b]])
        out = torch.full_like(audio, SENTINEL)
        tab = _table(eng, [[SLOTS[b], start + done[b], ln[b], 0] for b in range(4)])
        assert _embed(eng, audio, tab, pool, 5, out) == 0, eng.lib.smtts_last_error(eng.h)
        o = out.cpu().numpy()[:, 0]
        ph = pool.cpu().numpy()
        for b in range(4):
            want = refs[b].push(x[b, done[b]: done[b] + ln[b]])
            assert np.array_equal(_bits(o[b, :ln[b]]), _bits(want)), (c, b)
            assert (o[b, ln[b]:] == SENTINEL).all(), (c, b)
            assert np.array_equal(_bits(ph[SLOTS[b], :127]), _bits(refs[b].hist)), (c, b)       # the slot after every call
            got[b].append(o[b, :ln[b]].copy())
            done[b] += ln[b]
        assert (ph[4] == SENTINEL).all()
    assert done == list(LENS)
    # device chunked == device whole (one chunk on a fresh slot; without a pool too where the stream starts at 0)
    audio = torch.from_numpy(x[:, None]).to(eng.device)
    for pooled in ((True, False) if start == 0 else (True,)):
        out = torch.zeros_like(audio)
        fresh = torch.zeros(5, 128, device=eng.device) if pooled else None
        tab = _table(eng, [[SLOTS[b], start, LENS[b], 0] for b in range(4)])
        assert _embed(eng, audio, tab, fresh, 5 if pooled else 0, out) == 0
        o = out.cpu().numpy()[:, 0]
        for b, n in enumerate(LENS):
            assert np.array_equal(_bits(o[b, :n]), _bits(np.concatenate(got[b]))), (pooled, b)


def test_engine_watermark_streams_and_refuses_duplicate_slots(eng):
    x = _signal(2, 500, 3)
    audio = torch.from_numpy(x[:, None]).to(eng.device)
    st = eng.watermark_state(3)
    a = eng.watermark(audio[:, :, :200].contiguous(), [200, 130], KEY, STRENGTH, state=st, slots=[2, 0], n_before=[0, 0])
    b = eng.watermark(audio[:, :, 200:].contiguous(), [300, 0], KEY, STRENGTH, state=st, slots=[2, 0], n_before=[200, 130])
    got = np.concatenate([a.cpu().numpy()[0, 0], b.cpu().numpy()[0, 0]])
    assert np.array_equal(_bits(got), _bits(W.embed(x[0], KEY, STRENGTH)))
    assert np.array_equal(_bits(a.cpu().numpy()[1, 0, :130]), _bits(W.embed(x[1, :130], KEY, STRENGTH)))
    assert not st[1].any()
    with pytest.raises(ValueError, match="distinct slots"):
        eng.watermark(audio, [500, 500], KEY, STRENGTH, state=st, slots=[1, 1], n_before=[0, 0])
    with pytest.raises(ValueError, match="distinct slots"):
        eng.watermark(audio, [500, 500], KEY, STRENGTH, state=st, slots=[0, 3], n_before=[0, 0])
    with pytest.raises(ValueError, match="without state"):
        eng.watermark(audio, [500, 500], KEY, STRENGTH, n_before=[0, 5])
    with pytest.raises(ValueError, match="strength"):
        eng.watermark(audio, [500, 500], KEY, 1.5)
    with pytest.raises(ValueError, match="distinct slots"):
        eng.deliver(audio, [500, 500], 24000, "f32", slots=[1, 1], n_before=[0, 0], mark=(KEY, STRENGTH), mark_state=st)
    with pytest.raises(ValueError, match="mark_state"):
        eng.deliver(audio, [500, 500], 24000, "f32", mark_state=st)


# ---- 2. the detector -------------------------------------------------------------------------------------------------------------------
DLENS = (3000, 3, 1100)                           # two full tiles and a tail; almost nothing; one tile and a tail
DS = 3008
N_OFF = 300                                       # one full offset tile and a part


def _detect_signal(o_lo):
    """Three rows of speech-like audio, marked as streams that began 37 samples in front of o_lo (so the mark sits at offset o_lo + 37),
    NaN behind len."""
    sp = W.speechlike(0.4, seed=4)
    x = np.full((3, DS), np.nan, np.float32)
    for b, n in enumerate(DLENS):
        src = sp[2000 + 500 * b: 2000 + 500 * b + n + 37]
        y = W.Stream(KEY, 0.05, start=o_lo).push(src)
        x[b, :n] = y[37:]
    return x


def _detect(eng, audio, lens, key, o_lo, n_off, ws, ws_bytes, u, den, T, off, z, B=None, row=None):
    B = int(audio.shape[0]) if B is None else B
    row = int(audio.shape[1]) if row is None else row
    return eng.lib.smtts_watermark_detect(eng.h, eng._stream(), _p(audio), B, row, _p(lens), key, o_lo, n_off, _p(ws), ws_bytes, _p(u),
                                          _p(den), _p(T), _p(off), _p(z))


@pytest.fixture(scope="module")
def detect_refs():
    """o_lo -> (signal, [restatement per row]); computed once, never changed."""
    out = {}
    for o_lo in (0, 2 ** 33 + 5, 2 ** 39 + 5):
        x = _detect_signal(o_lo)
        out[o_lo] = (x, [W.detect(x[b, :n], KEY, o_lo, N_OFF) for b, n in enumerate(DLENS)])
    return out


@pytest.mark.parametrize("o_lo", [0, 2 ** 33 + 5, 2 ** 39 + 5])
def test_detector_against_the_fp64_restatement(eng, detect_refs, o_lo):
    x, refs = detect_refs[o_lo]
    T, den, off, z, u = [t.cpu().numpy() for t in eng.watermark_detect(torch.from_numpy(x).to(eng.device), DLENS, KEY, o_lo=o_lo,
                                                                        n_off=N_OFF, return_u=True)]
    T2, den2, off2, z2 = [t.cpu().numpy() for t in eng.watermark_detect(torch.from_numpy(x).to(eng.device), DLENS, KEY, o_lo=o_lo,
                                                                        n_off=N_OFF)]
    assert np.array_equal(_bits(T), _bits(T2)) and np.array_equal(_bits(den), _bits(den2)) and np.array_equal(off, off2)   # two calls
    assert np.array_equal(_bits(z), _bits(z2))
    for b, n in enumerate(DLENS):
        r = refs[b]
        # u: the per-sample bound counted next to the restatement
        err = np.abs(u[b, :n].astype(np.float64) - r["u"])
        worst = float((err / r["bound"]).max()) if n else 0.0
        print(f"o_lo {o_lo} row {b} (len {n}): u err / bound max {worst:.3f}, max |u| {np.abs(r['u']).max():.3e}")
        assert (err <= r["bound"]).all(), (b, worst)
        assert not u[b, n:].any()                                                    # written below len only
        # T and den: fp64 sums of the device's OWN u, within what the stated order allows
        ud = u[b, :n].astype(np.float64)
        Tref = W.correlate(ud, KEY, o_lo, N_OFF)
        tb = W.t_bound(float(np.abs(ud).sum()), n)
        print(f"    T err / bound max {float(np.abs(T[b] - Tref).max() / max(tb, 1e-300)):.3f}, "
              f"den err / bound {abs(float(den[b]) - float((ud * ud).sum())) / max(W.den_bound(float((ud * ud).sum()), n), 1e-300):.3f}")
        assert (np.abs(T[b].astype(np.float64) - Tref) <= tb).all(), b
        assert abs(float(den[b]) - float((ud * ud).sum())) <= W.den_bound(float((ud * ud).sum()), n), b
        # best_off, best_z: integer logic and single fp32 operations on the device's T and den, exactly
        k = int(np.argmax(T[b]))                                                     # numpy: the first of equal maxima
        assert int(off[b]) == o_lo + k, b
        want_z = np.float32(0.0) if den[b] == 0 else np.float32(T[b, k]) / np.sqrt(np.float32(den[b]))
        assert _bits([z[b]])[0] == _bits([want_z])[0], b
    assert int(off[0]) == o_lo + 37 and z[0] > 12 and int(off[2]) == o_lo + 37 and z[2] > 12   # (the mark is where it was put)
    assert den[1] == 0 and z[1] == 0 and int(off[1]) == o_lo and not T[1].any()      # r reads as 0 below 33 samples: no evidence, the lowest offset


def test_detector_rows_are_isolated_and_nothing_behind_len_is_read(eng, detect_refs):
    o_lo = 2 ** 33 + 5
    x, _refs = detect_refs[o_lo]
    base = [t.cpu().numpy() for t in eng.watermark_detect(torch.from_numpy(x).to(eng.device), DLENS, KEY, o_lo=o_lo, n_off=N_OFF,
                                                          return_u=True)]
    other = x.copy()
    other[np.isnan(other)] = 3.0                                                      # other bytes behind len
    other[1] = 0.25                                                                   # another batch-mate (row 1 whole)
    got = [t.cpu().numpy() for t in eng.watermark_detect(torch.from_numpy(other).to(eng.device), [DLENS[0], DS, DLENS[2]], KEY,
                                                         o_lo=o_lo, n_off=N_OFF, return_u=True)]
    for a, g in zip(base, got):
        for b in (0, 2):
            assert np.array_equal(np.ascontiguousarray(a[b]).view(np.uint8), np.ascontiguousarray(g[b]).view(np.uint8)), b
    for b in (0, 2):                                                                  # ... and alone, at another row stride
        n = DLENS[b]
        alone = [t.cpu().numpy() for t in eng.watermark_detect(torch.from_numpy(x[b: b + 1, : n]).contiguous().to(eng.device), [n], KEY,
                                                               o_lo=o_lo, n_off=N_OFF, return_u=True)]
        for a, g in zip(base[:4], alone[:4]):
            assert np.array_equal(np.ascontiguousarray(a[b]).view(np.uint8), np.ascontiguousarray(g[0]).view(np.uint8)), b
        assert np.array_equal(_bits(base[4][b, :n]), _bits(alone[4][0]))


# ---- 3. guard bands and refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooled", [False, True])
def test_embedder_between_guard_bands(eng, pooled):
    x = _signal(4, 261, 5)
    lens = [1, 64, 200, 261]
    for b, n in enumerate(lens):
        x[b, n:] = np.nan
    ar = Arena("cuda")
    audio = ar.put("audio", torch.from_numpy(x[:, None]))
    table = ar.put("table", torch.tensor([[s, a, n, 0] for s, a, n in zip(SLOTS, [0, 37, 2 ** 33 + 5, 1000], lens)], dtype=torch.int64))
    pool0 = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (4, 128)).astype(np.float32))
    pool = ar.put("pool", pool0) if pooled else None
    out = ar.alloc("out", (4, 1, 261), torch.float32, skew=4)
    res = []
    for byte in (0x00, 0xFF):
        if pooled:
            pool.copy_(pool0)
        ar.paint(byte)
        assert _embed(eng, audio, table, pool, 4 if pooled else 0, out) == 0, eng.lib.smtts_last_error(eng.h)
        torch.cuda.synchronize()
        ar.assert_clean("smtts_watermark", (pooled, byte))
        res.append((out.cpu().numpy().copy(), None if pool is None else pool.cpu().numpy().copy()))
    assert np.array_equal(res[0][0].view(np.uint8), res[1][0].view(np.uint8))
    if pooled:
        assert np.array_equal(res[0][1].view(np.uint8), res[1][1].view(np.uint8))
        assert np.array_equal(res[0][1][:, 127], pool0.numpy()[:, 127])             # the slot's padding word is not touched
    for b, n in enumerate(lens):
        assert not res[0][0][b, 0, n:].view(np.uint8).any() and np.isfinite(res[0][0][b, 0, :n]).all(), b


@pytest.mark.parametrize("own_u", [False, True])
def test_detector_between_guard_bands(eng, detect_refs, own_u):
    x, _refs = detect_refs[0]
    ar = Arena("cuda")
    audio = ar.put("audio", torch.from_numpy(x))
    lens = ar.put("len", torch.tensor(DLENS, dtype=torch.int64))
    need = int(eng.lib.smtts_watermark_detect_workspace_bytes(eng.h, 3, DS))
    assert need == -(-3 * DS * 4 // 256) * 256 + 256                                 # u's place and 3 x 3 tile sums, each rounded up to 256
    ws = ar.workspace("ws", need)
    u = ar.alloc("u", (3, DS), torch.float32) if own_u else None
    den, z = ar.alloc("den", (3,), torch.float32), ar.alloc("z", (3,), torch.float32)
    T = ar.alloc("T", (3, N_OFF), torch.float32, skew=4)
    off = ar.alloc("off", (3,), torch.int64)
    res = []
    for byte in (0x00, 0xFF):
        ar.paint(byte)
        assert _detect(eng, audio, lens, KEY, 5, N_OFF, ws, need, u, den, T, off, z) == 0, eng.lib.smtts_last_error(eng.h)
        torch.cuda.synchronize()
        ar.assert_clean("smtts_watermark_detect", (own_u, byte))
        res.append([t.cpu().numpy().copy() for t in (den, T, off, z) + ((u,) if own_u else ())])
    for a, b in zip(*res):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert np.isfinite(res[0][1]).all() and res[0][0][0] > 0
    if own_u:
        assert all(not res[0][4][b, n:].any() for b, n in enumerate(DLENS))
    # one byte less of workspace is refused
    assert _detect(eng, audio, lens, KEY, 5, N_OFF, ws, need - 1, u, den, T, off, z) == 1
    assert b"smtts_watermark_detect" in eng.lib.smtts_last_error(eng.h)


def test_bad_arguments_are_refused_before_anything_is_enqueued(eng):
    lib = eng.lib
    ar = Arena("cuda")
    audio = ar.put("audio", torch.from_numpy(_signal(2, 64, 0)[:, None]))
    table = ar.put("table", torch.tensor([[0, 0, 64, 1], [1, 0, 64, 1]], dtype=torch.int64))
    pool = ar.alloc("pool", (2, 512), torch.uint8, role="in")
    pool.zero_()
    out = ar.alloc("out", (2, 1, 64), torch.float32)
    ok = dict(audio=audio, B=2, row=64, table=table, strength=STRENGTH, pool=pool, n_slots=2, out=out)
    skewed = pool.view(-1)[4:4 + 512]
    bad = [dict(B=0), dict(B=65536), dict(audio=None), dict(table=None), dict(out=None), dict(row=0), dict(row=2 ** 40 + 1),
           dict(strength=-0.01), dict(strength=1.01), dict(strength=float("nan")), dict(strength=float("inf")), dict(pool=skewed),
           dict(n_slots=0), dict(out=audio), dict(out=audio.view(-1)[32:], B=1)]
    ar.paint(0xFF)
    for kw in bad:
        a = dict(ok, **kw)
        rc = _embed(eng, a["audio"], a["table"], a["pool"], a["n_slots"], a["out"], strength=a["strength"], B=a["B"], row=a["row"])
        assert rc == 1 and b"smtts_watermark" in lib.smtts_last_error(eng.h), kw
    torch.cuda.synchronize()
    ar.assert_clean("smtts_watermark", "refusals")
    assert not out.any() and not pool.any()
    assert _embed(eng, audio, table, pool, 2, out) == 0
    torch.cuda.synchronize()
    ar.assert_clean("smtts_watermark", "good")
    # the detector
    lens = ar.put("len", torch.tensor([64, 64], dtype=torch.int64))
    need = int(lib.smtts_watermark_detect_workspace_bytes(eng.h, 2, 64))
    assert lib.smtts_watermark_detect_workspace_bytes(eng.h, 0, 64) == 0 and lib.smtts_watermark_detect_workspace_bytes(eng.h, 1025, 64) == 0
    assert lib.smtts_watermark_detect_workspace_bytes(eng.h, 1, 0) == 0
    ws = ar.workspace("ws", need)
    den, z, T, off = (ar.alloc("den", (2,), torch.float32), ar.alloc("z", (2,), torch.float32), ar.alloc("T", (2, 8), torch.float32),
                      ar.alloc("off", (2,), torch.int64))
    a2 = audio.view(2, 64)
    okd = dict(audio=a2, B=2, row=64, lens=lens, o_lo=0, n_off=8, ws=ws, ws_bytes=need, den=den, T=T, off=off, z=z)
    badd = [dict(B=0), dict(B=1025), dict(row=0), dict(audio=None), dict(lens=None), dict(ws=None), dict(den=None), dict(T=None),
            dict(off=None), dict(z=None), dict(o_lo=-1), dict(o_lo=2 ** 40 + 1), dict(n_off=0), dict(n_off=65537), dict(ws=ws[4:]),
            dict(ws_bytes=need - 1)]
    ar.paint(0xFF)
    for kw in badd:
        a = dict(okd, **kw)
        rc = _detect(eng, a["audio"], a["lens"], KEY, a["o_lo"], a["n_off"], a["ws"], a["ws_bytes"], None, a["den"], a["T"], a["off"], a["z"],
                     B=a["B"], row=a["row"])
        assert rc == 1 and b"smtts_watermark_detect" in lib.smtts_last_error(eng.h), kw
    torch.cuda.synchronize()
    ar.assert_clean("smtts_watermark_detect", "refusals")
    assert not T.any() and not den.any()
    assert _detect(eng, a2, lens, KEY, 0, 8, ws, need, None, den, T, off, z) == 0
    torch.cuda.synchronize()
    ar.assert_clean("smtts_watermark_detect", "good")


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------------
REF = torch.randn(5, 64, generator=torch.Generator().manual_seed(0)).numpy()
TOKS, DUR, N = [3, 17, 42, 99, 150, 7, 8], 1.7, 12
WM_KEY = 0xA11CE


def _z_interval(audio, key, o, z_ref_row):
    """The restatement's z(o) of `audio` and the interval the device's z must lie in: T and den move by the u bound summed and by the
    summation bounds of test 2, z = T / sqrt(den) by one fp32 square root and one division on top."""
    r = W.detect(audio, key, o, 1)
    n = len(audio)
    au = np.abs(r["u"]) + r["bound"]                                                 # |device u| <= this
    dT = float(r["bound"].sum()) + W.t_bound(float(au.sum()), n)
    dden = float((2 * np.abs(r["u"]) * r["bound"] + r["bound"] ** 2).sum()) + W.den_bound(float((au * au).sum()), n)
    T, den = float(r["T"][0]), r["den"]
    if den - dden <= 0:
        return r, -np.inf, np.inf
    cands = [t / np.sqrt(d) for t in (T - dT, T + dT) for d in (den - dden, den + dden)]
    slack = 3 * W.U * max(abs(c) for c in cands)
    return r, min(cands) - slack, max(cands) + slack


def _check_detect(tts, marked, key, what):
    """detect_watermark on the marked audio (f32 or int16) == the restatement's z at offset 0, within test 2's bounds; no absolute bar."""
    y = marked.reshape(-1)
    yf = y.astype(np.float32) / np.float32(32767.0) if y.dtype == np.int16 else y
    r, lo, hi = _z_interval(yf, key, 0, None)
    (z, off, present), = tts.detect_watermark(marked, key)
    print(f"[{what}] device z {z:.3f}, restatement {r['z'][0]:.3f}, interval [{lo:.3f}, {hi:.3f}]")
    assert off == 0 and lo <= z <= hi and present == (z >= 6.0), what
    return z


def test_synthesize_stream_and_decode_stream_mark_the_chunks(eng):
    from smalltts_amd.api import Decoder, Delivery, SmallTTS, Watermark
    tts = SmallTTS(engine=eng, seed=0)
    wm = Watermark(WM_KEY)
    plain = list(tts.synthesize_stream(REF, TOKS, DUR, seed=77))
    again = list(tts.synthesize_stream(REF, TOKS, DUR, seed=77, watermark=None))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(plain, again))   # without watermark=: as before
    audio = np.concatenate(plain, axis=1)[0]
    want = W.embed(audio, WM_KEY, 0.02)
    assert audio.shape == (3200 * N,) and not np.array_equal(want, audio)
    got = list(tts.synthesize_stream(REF, TOKS, DUR, seed=77, watermark=wm))         # without deliver=: Delivery(24000, "f32")
    assert [g.shape for g in got] == [p.shape for p in plain] and got[0].dtype == np.float32
    assert np.array_equal(_bits(np.concatenate(got, axis=1)[0]), _bits(want))
    got16 = list(tts.synthesize_stream(REF, TOKS, DUR, seed=77, watermark=(WM_KEY, 0.02), deliver=Delivery(24000, "pcm16")))
    cat16 = np.concatenate(got16, axis=1)
    assert cat16.dtype == np.int16 and np.array_equal(cat16[0], DR.pcm16(want))
    # the whole call: synthesize_batch marks each row as a stream of its own; the chunked decode differs from the whole decode by
    # fp32 summation order, so the whole call is held to its own unmarked result
    whole_plain = tts.synthesize_batch([REF], [TOKS], [DUR], seeds=[77])[0]
    whole = tts.synthesize_batch([REF], [TOKS], [DUR], seeds=[77], watermark=wm)[0]
    assert np.array_equal(_bits(whole[0]), _bits(W.embed(whole_plain[0], WM_KEY, 0.02)))
    _check_detect(tts, np.concatenate(got, axis=1), WM_KEY, "synthesize_stream f32")
    _check_detect(tts, cat16, WM_KEY, "synthesize_stream pcm16")
    # DecodeStream: the mark slot next to the decode slot, rewound and reset with it
    lat = torch.from_numpy(np.concatenate([l for _, l in tts.synthesize_stream(REF, TOKS, DUR, seed=77, return_latents=True)])[None])
    st = Decoder(engine=eng).open_stream(rows=1, watermark=wm)
    a = st.decode(lat[:, :2])
    snap = st.snapshot()
    b = st.decode(lat[:, 2:6])
    c = st.decode(lat[:, 6:], last=True)
    assert np.array_equal(_bits(torch.cat([a, b, c], dim=1).numpy()[0]), _bits(want))
    st.restore(snap)
    assert torch.equal(st.decode(lat[:, 2:6]), b)
    st.reset()
    assert torch.equal(st.decode(lat[:, :2]), a)
    un = Decoder(engine=eng).open_stream(rows=1)
    assert np.array_equal(_bits(un.decode(lat[:, :2]).numpy()[0, 0]), _bits(audio[:6400]))   # without watermark=: as before


def test_synthesize_long_and_long_stream_mark_the_joined_waveform(eng):
    from smalltts_amd.api import Delivery, SmallTTS
    tts = SmallTTS(engine=eng, seed=0)
    voice = tts.encode_voice(REF)
    kw = dict(token_lists=[TOKS, TOKS[:4], TOKS[2:], TOKS[1:5], TOKS[:6]], durations=[0.3, 0.6, 0.4, 0.3, 0.4], seed=3, max_batch=2,
              in_flight=2, gap_ms=20.0, fade_ms=2.0)
    plain = tts.synthesize_long(voice, **kw)
    assert np.array_equal(tts.synthesize_long(voice, watermark=None, **kw).view(np.uint32), plain.view(np.uint32))
    want = W.embed(plain[0], WM_KEY, 0.02)
    got = tts.synthesize_long(voice, watermark=WM_KEY, **kw)
    assert got.dtype == np.float32 and np.array_equal(_bits(got[0]), _bits(want))
    got16 = tts.synthesize_long(voice, watermark=WM_KEY, deliver=Delivery(24000, "pcm16"), **kw)
    assert got16.dtype == np.int16 and np.array_equal(got16[0], DR.pcm16(want))
    _check_detect(tts, got, WM_KEY, "synthesize_long f32")
    _check_detect(tts, got16, WM_KEY, "synthesize_long pcm16")
    # streamed, the default ramp: the chunks are the mark of the un-marked chunks' concatenation, whatever the grouping ...
    s_plain = [c.audio for c in tts.synthesize_long_stream(voice, **kw)]
    s_none = [c.audio for c in tts.synthesize_long_stream(voice, watermark=None, **kw)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(s_plain, s_none))
    for dv, enc in ((None, None), (Delivery(24000, "pcm16"), "pcm16")):
        chunks = list(tts.synthesize_long_stream(voice, watermark=WM_KEY, **({} if dv is None else {"deliver": dv}), **kw))
        assert [c.audio.shape for c in chunks] == [a.shape for a in s_plain] and len(chunks) == 3
        s_want = W.embed(np.concatenate(s_plain, axis=1)[0], WM_KEY, 0.02)
        cat = np.concatenate([c.audio for c in chunks], axis=1)[0]
        assert np.array_equal(cat, DR.pcm16(s_want)) if enc else np.array_equal(_bits(cat), _bits(s_want)), enc
        pos = 0
        for c in chunks:
            assert c.offset == pos
            pos += c.audio.shape[1]
    _check_detect(tts, cat[None], WM_KEY, "synthesize_long_stream pcm16")
    # ... and in synthesize_long's own groups the stream's chunks concatenate to the whole call's bytes
    same = np.concatenate([c.audio for c in tts.synthesize_long_stream(voice, watermark=WM_KEY, batch_sizes=None, **kw)], axis=1)
    assert same.tobytes() == got.tobytes()
    # another key, and the un-marked audio, are the same evidence as in the restatement
    _check_detect(tts, got, WM_KEY + 1, "synthesize_long f32, another key")
    _check_detect(tts, plain, WM_KEY, "synthesize_long unmarked")
    # a cropped copy is found at its offset where the restatement finds it
    crop = 1003
    r = W.detect(got[0, crop:], WM_KEY, 0, 1100)
    (z, off, present), = tts.detect_watermark(got[0, crop:], WM_KEY, max_offset=1099)
    print(f"[cropped by {crop}] device z {z:.3f} at {off}; restatement {r['best_z']:.3f} at {r['best_off']}")
    if r["best_z"] > 2 * np.sort(r["z"])[-2] and r["best_z"] > 6:                    # a clear peak in the restatement: the device names it too
        assert off == r["best_off"]
    many = tts.detect_watermark([got[0], got16[0], plain[0, :100]], WM_KEY)
    assert len(many) == 3 and many[0][1] == 0
