"""GPU: delivery (include/smalltts_hip.h smtts_deliver): the kernel against the fp64 restatement of tests/helpers/deliver_ref.py
at the fp32 summation bound, chunked delivery against whole delivery bit for bit with the carried history checked after every call, the
pass-through rate against engine.pcm16 and audioop's G.711 codes, the production bank once, guard bands and refusals, and the public
layers on top (synthesize_batch, synthesize_stream, the server).

Test banks have zeros=3 (44.1 kHz: up 147, down 80, width 4, klen 88; 8 kHz: width 10, klen 23); the 8 kHz chunk splits are also run on
the zeros=1 bank, whose width 4, klen 11 and H 10 are what the splits [3, 10, 11, n - 24] aim at (a chunk of exactly H and of exactly
klen samples)."""
import ctypes as C

import numpy as np
import pytest
import torch

from smalltts_amd import audio as A
from tests.conftest import golden
from tests.helpers import deliver_ref as R
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
DT = (torch.float32, torch.int16, torch.uint8, torch.uint8)
ENC = A.DELIVER_ENCODINGS


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    from tests.test_stream_gpu import API_SEED, API_SPEC
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(API_SEED, parts=("dit", "decoder", "encoder"), codec_spec=API_SPEC)
    e.finalize()
    return e


def _bank(rate, zeros):
    up, down = A.deliver_ratio(rate)
    k, width = A._sinc_kernel(down, up, zeros)
    return k, up, down, width


def _signal(B, S, seed):
    """noise at 0.5 amplitude, and samples of +-4 in row 0 (the encoders' clamp)"""
    x = (0.5 * np.random.default_rng(seed).uniform(-1.0, 1.0, (B, 1, S))).astype(np.float32)
    x[0, 0, ::7] = 4.0
    x[0, 0, 3::11] = -4.0
    return x


def _lens(rate, which):
    _k, up, down, width = _bank(rate, 3)
    return ([1, width + down, 257], [down - 1, width, 50])[which]


# ---- 1. whole signals against fp64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("rate", [8000, 16000, 48000, 44100])
def test_whole_delivery_is_the_fp64_restatement_within_the_fp32_summation_bound(eng, rate, which):
    bank, up, down, width = _bank(rate, 3)
    klen = bank.shape[1]
    lens = _lens(rate, which)
    x = _signal(3, 260, rate + which)
    xd = torch.from_numpy(x).to(eng.device)
    out, counts = eng.deliver(xd, lens, rate, "f32", zeros=3)
    assert counts == A.deliver_counts([0] * 3, lens, True, up, down, width) == [-(-up * n // down) for n in lens]
    got = out.cpu().numpy()
    for b, n in enumerate(lens):
        want, mag = R.deliver_whole(x[b, 0, :n], bank, down, width)
        err = np.abs(got[b, :counts[b]].astype(np.float64) - want)
        bound = R.fp32_bound(mag, klen)
        print(f"\n[deliver] {rate} Hz row {b} len {n}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0:.3f}")
        assert (err <= bound).all()
    for e in (1, 2, 3):
        o, c = eng.deliver(xd, lens, rate, ENC[e], zeros=3)
        assert c == counts and o.dtype == DT[e]
        o = o.cpu().numpy()
        for b in range(3):
            assert np.array_equal(o[b, :c[b]], R.encode(got[b, :c[b]], e)), (rate, e, b)


# ---- 2. chunked equals whole, bit for bit ---------------------------------------------------------------------------------------------
def _splits(n):
    return ([n], [1] * n, [3, 10, 11, n - 24], [9, 1, n - 10], [n, 0])


@pytest.mark.parametrize("enc", [0, 1, 2, 3])
@pytest.mark.parametrize("rate,zeros,n", [(8000, 3, 50), (8000, 1, 50), (44100, 3, 257)])
def test_chunked_delivery_is_whole_delivery_bit_for_bit(eng, rate, zeros, n, enc):
    """Two streams in one pool (slots 3 and 1 of 5): stream A walks one split, stream B the next one, so the rows of a call advance by
    different lengths, one stream ends earlier and is left out of the later calls.  After every call both slots hold the restated
    history bit for bit and the other slots are still zero."""
    bank, up, down, width = _bank(rate, zeros)
    klen = bank.shape[1]
    x = _signal(2, n, 7 * n + zeros)
    xd = torch.from_numpy(x).to(eng.device)
    whole, wc = eng.deliver(xd, [n, n], rate, ENC[enc], zeros=zeros)
    whole = whole.cpu().numpy()
    assert wc == [-(-up * n // down)] * 2
    sp = _splits(n)
    for i, split_a in enumerate(sp):
        split_b = sp[(i + 1) % len(sp)]
        state = eng.deliver_state(5, rate, zeros)
        assert state.shape[1] == (4 * (klen - 1) + 255) // 256 * 256
        refs = [R.Stream(bank, down, width), R.Stream(bank, down, width)]
        pos, got = [0, 0], [[], []]
        for k in range(max(len(split_a), len(split_b))):
            rows = [r for r, s in enumerate((split_a, split_b)) if k < len(s)]
            ln = [(split_a, split_b)[r][k] for r in rows]
            last = [k == len((split_a, split_b)[r]) - 1 for r in rows]
            S = max(max(ln), 1) + 3                                         # row_stride larger than every len
            chunk = torch.zeros(len(rows), 1, S)
            for j, r in enumerate(rows):
                chunk[j, 0, :ln[j]] = torch.from_numpy(x[r, 0, pos[r]:pos[r] + ln[j]])
            out, cnt = eng.deliver(chunk.to(eng.device), ln, rate, ENC[enc], state=state, slots=[(3, 1)[r] for r in rows],
                                   n_before=[pos[r] for r in rows], last=last, zeros=zeros)
            out, st = out.cpu().numpy(), state.cpu().numpy()
            for j, r in enumerate(rows):
                o_lo, o_hi = refs[r].advance(x[r, 0, pos[r]:pos[r] + ln[j]], last[j])
                assert cnt[j] == o_hi - o_lo
                got[r].append(out[j, :cnt[j]])
                pos[r] += ln[j]
                hist = st[(3, 1)[r], :4 * (klen - 1)].view(np.float32)
                assert np.array_equal(hist.view(np.uint32), refs[r].hist.view(np.uint32)), (split_a, split_b, k, r)
            assert not st[[0, 2, 4]].any()
        for r in range(2):
            cat = np.concatenate(got[r])
            assert cat.size == wc[r] and np.array_equal(cat.view(np.uint8), whole[r, :wc[r]].view(np.uint8)), (split_a, split_b, r)


def test_a_slot_can_be_rewound_and_is_read(eng):
    rate, n = 44100, 257
    bank, up, down, width = _bank(rate, 3)
    x = torch.from_numpy(_signal(1, n, 1)).to(eng.device)
    state = eng.deliver_state(1, rate, 3)
    eng.deliver(x[:, :, :100].contiguous(), [100], rate, "f32", state=state, slots=[0], n_before=[0], last=False, zeros=3)
    snap = state.clone()
    kw = dict(state=state, slots=[0], n_before=[100], last=False, zeros=3)
    a, ca = eng.deliver(x[:, :, 100:257].contiguous(), [157], rate, "f32", **kw)
    assert not torch.equal(state, snap)
    state.copy_(snap)
    b, cb = eng.deliver(x[:, :, 100:257].contiguous(), [157], rate, "f32", **kw)
    assert ca == cb and ca[0] > 0 and torch.equal(a[:, :ca[0]], b[:, :cb[0]])
    state.zero_()                                                           # a zeroed slot mid-stream: the history is gone
    c, cc = eng.deliver(x[:, :, 100:257].contiguous(), [157], rate, "f32", **kw)
    assert cc == ca and not torch.equal(a[:, :ca[0]], c[:, :cc[0]])


# ---- 3. the pass-through rate -----------------------------------------------------------------------------------------------------------
def test_pass_through_is_pcm16_and_audioops_g711_codes(eng):
    x = torch.from_numpy(_signal(2, 1001, 3)).to(eng.device)
    out, cnt = eng.deliver(x, [1001, 77], 24000, "pcm16")
    assert cnt == [1001, 77]
    want = eng.pcm16(x)[:, 0]
    assert torch.equal(out[0], want[0]) and torch.equal(out[1, :77], want[1, :77])
    f, cnt = eng.deliver(x, [1001, 77], 24000, "f32")
    assert torch.equal(f[0], x[0, 0]) and torch.equal(f[1, :77], x[1, 0, :77])
    s = np.arange(-32768, 32768, dtype=np.int32)
    v = torch.from_numpy((s / 32767.0).astype(np.float32)).view(1, 1, -1).to(eng.device)
    keep = s >= -32767                                                      # -32768 / 32767 clamps to -32767: the one value not reachable
    assert np.array_equal(eng.pcm16(v).cpu().numpy().reshape(-1)[keep], s[keep].astype(np.int16))
    codes = golden("g711_codes.npz")
    for e, law in ((2, "mulaw"), (3, "alaw")):
        got = eng.deliver(v, [65536], 24000, ENC[e])[0].cpu().numpy().reshape(-1)
        assert np.array_equal(got[keep], codes[law][keep]), law
        assert got[0] == codes[law][1]                                      # s = -32768 arrives as -32767


# ---- 4. the production bank once ----------------------------------------------------------------------------------------------------------
def test_production_bank_at_8_khz_against_fp64_and_resample_poly(eng):
    bank_d, up, down, width, klen = eng.deliver_bank(8000)
    assert (up, down, width, klen) == (1, 3, 205, 413) and A.DELIVER_ZEROS == 64
    bank = bank_d.cpu().numpy()
    n = 6400
    x = _signal(1, n, 9)
    xd = torch.from_numpy(x).to(eng.device)
    out, cnt = eng.deliver(xd, [n], 8000, "f32")
    assert cnt == [2134]
    got = out.cpu().numpy()[0, :cnt[0]]
    want, mag = R.deliver_whole(x[0, 0], bank, down, width)
    bound = R.fp32_bound(mag, klen)
    assert (np.abs(got.astype(np.float64) - want) <= bound).all()
    y = torch.empty(1, cnt[0], device=eng.device)
    rc = eng.lib.smtts_resample_poly(eng.h, eng._stream(), _p(xd), 1, n, _p(bank_d), up, down, klen, width, _p(y), cnt[0])
    assert rc == 0
    assert (np.abs(got.astype(np.float64) - y.cpu().numpy()[0].astype(np.float64)) <= 2 * bound).all()


# ---- 5. guard bands and refusals ------------------------------------------------------------------------------------------------------
def _call(eng, audio, B, row_stride, table, bank, up, down, klen, width, pool, n_slots, enc, out, out_stride):
    return eng.lib.smtts_deliver(eng.h, eng._stream(), _p(audio), B, row_stride, _p(table), _p(bank), up, down, klen, width,
                                 _p(pool), n_slots, enc, _p(out), out_stride)


@pytest.mark.parametrize("enc", [0, 1, 2, 3])
@pytest.mark.parametrize("rate", [8000, 16000, 48000, 44100, 24000])
def test_nothing_is_written_or_read_outside_the_buffers(eng, rate, enc):
    """The odd shapes of test 1, `out` at a 4-byte-skewed address, row_stride larger than every len, streamed (a pool) and whole.  What
    lies behind len[b] in a row is NaN and the guards are painted 0x00 and 0xFF: the results must not change, nothing behind cnt_b is
    written (the output payload is zeroed by every paint), and no guard byte changes."""
    if rate == 24000:
        bank, up, down, width, klen = None, 1, 1, 0, 0
        lens = [1, 9, 257]
    else:
        bank, up, down, width = _bank(rate, 3)
        klen = bank.shape[1]
        lens = _lens(rate, 0)
    S = 261
    x = _signal(3, S, rate)
    for b, n in enumerate(lens):
        x[b, 0, n:] = np.nan
    for pooled in ((False,) if bank is None else (False, True)):
        nb = [0, 0, 0] if not pooled else [0, 37, 1000]
        last = [1, 1, 1] if not pooled else [0, 1, 0]
        counts = lens if bank is None else A.deliver_counts(nb, lens, last, up, down, width)
        stride = A.deliver_max_count(S, up, down, width, pooled)
        ar = Arena("cuda")
        audio = ar.put("audio", torch.from_numpy(x))
        table = ar.put("table", torch.tensor([[s, a, n, f] for s, a, n, f in zip([2, 0, 1], nb, lens, last)], dtype=torch.int64))
        bank_d = None if bank is None else ar.put("bank", torch.from_numpy(bank))
        pool0 = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (3, 64 * ((klen - 1 + 63) // 64))).astype(np.float32)) if pooled else None
        pool = ar.put("pool", pool0) if pooled else None
        out = ar.alloc("out", (3, stride), DT[enc], skew=4)
        res = []
        for byte in (0x00, 0xFF):
            if pooled:
                pool.copy_(pool0)
            ar.paint(byte)
            rc = _call(eng, audio, 3, S, table, bank_d, up, down, klen, width, pool, 3 if pooled else 0, enc, out, stride)
            assert rc == 0, eng.lib.smtts_last_error(eng.h)
            torch.cuda.synchronize()
            ar.assert_clean("smtts_deliver", (rate, enc, pooled, byte))
            res.append((out.cpu().numpy().copy(), None if pool is None else pool.cpu().numpy().copy()))
        o = res[0][0]
        assert np.array_equal(o.view(np.uint8), res[1][0].view(np.uint8))
        if pooled:
            assert np.array_equal(res[0][1].view(np.uint32), res[1][1].view(np.uint32))
        for b in range(3):
            assert not o[b, counts[b]:].view(np.uint8).any(), (rate, enc, pooled, b)       # nothing behind cnt_b
            assert np.isfinite(o[b, :counts[b]].astype(np.float64)).all()                  # nothing behind len[b] was read


def test_bad_arguments_are_refused_before_anything_is_enqueued(eng):
    bank, up, down, width = _bank(8000, 3)
    klen = bank.shape[1]
    ar = Arena("cuda")
    audio = ar.put("audio", torch.from_numpy(_signal(2, 64, 0)))
    table = ar.put("table", torch.tensor([[0, 0, 64, 1], [1, 0, 64, 1]], dtype=torch.int64))
    bank_d = ar.put("bank", torch.from_numpy(bank))
    pool = ar.alloc("pool", (2, 256), torch.uint8, role="in")
    pool.zero_()
    stride = A.deliver_max_count(64, up, down, width, True)
    out = ar.alloc("out", (2, stride), torch.float32)
    ok = dict(audio=audio, B=2, row_stride=64, table=table, bank=bank_d, up=up, down=down, klen=klen, width=width, pool=pool, n_slots=2, enc=0, out=out,
              out_stride=stride)
    lib = eng.lib
    assert lib.smtts_deliver_state_bytes(eng.h, klen) == 256 and lib.smtts_deliver_state_bytes(eng.h, 1) == 0
    assert lib.smtts_deliver_state_bytes(eng.h, 0) == 0 and lib.smtts_deliver_state_bytes(eng.h, 1 << 20) == 0
    skewed = pool.view(-1)[4:4 + 256]
    bad = [dict(B=0), dict(audio=None), dict(table=None), dict(out=None), dict(up=0), dict(down=0), dict(klen=klen + 1), dict(width=width + 1),
           dict(bank=None), dict(bank=None, pool=None, klen=0, width=0), dict(bank=None, up=1, down=1, klen=0, width=0),
           dict(pool=skewed), dict(n_slots=0), dict(enc=-1), dict(enc=4), dict(out_stride=stride - 1),
           dict(pool=None, n_slots=0, out_stride=-(-up * 64 // down) - 1), dict(row_stride=0)]
    ar.paint(0xFF)
    for kw in bad:
        a = dict(ok, **kw)
        rc = _call(eng, a["audio"], a["B"], a["row_stride"], a["table"], a["bank"], a["up"], a["down"], a["klen"], a["width"], a["pool"],
                   a["n_slots"], a["enc"], a["out"], a["out_stride"])
        assert rc == 1 and b"smtts_deliver" in lib.smtts_last_error(eng.h), kw
    torch.cuda.synchronize()
    ar.assert_clean("smtts_deliver", "refusals")
    assert not out.any()
    # the good call goes through, and so does the whole form (no pool) with its smaller out_stride
    assert _call(eng, audio, 2, 64, table, bank_d, up, down, klen, width, pool, 2, 0, out, stride) == 0
    assert _call(eng, audio, 2, 64, table, bank_d, up, down, klen, width, None, 0, 0, out, -(-up * 64 // down)) == 0
    torch.cuda.synchronize()
    ar.assert_clean("smtts_deliver", "good")
    with pytest.raises(ValueError, match="distinct slots"):
        eng.deliver(audio, [64, 64], 8000, "f32", state=eng.deliver_state(2, 8000, 3), slots=[1, 1], n_before=[0, 0], zeros=3)
    with pytest.raises(ValueError, match="distinct slots"):
        eng.deliver(audio, [64, 64], 8000, "f32", state=eng.deliver_state(2, 8000, 3), slots=[0, 2], n_before=[0, 0], zeros=3)
    with pytest.raises(ValueError, match="without state"):
        eng.deliver(audio, [64, 64], 8000, "f32", n_before=[0, 5], zeros=3)
    with pytest.raises(ValueError, match="encoding"):
        eng.deliver(audio, [64, 64], 8000, "s16", zeros=3)
    with pytest.raises(ValueError, match="rate"):
        eng.deliver(audio, [64, 64], 12000, "f32")


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------
REF = torch.randn(5, 64, generator=torch.Generator().manual_seed(0)).numpy()
TOKS, DUR, N = [3, 17, 42, 99, 150, 7, 8], 1.7, 12


def test_synthesize_batch_delivers_what_engine_deliver_makes_of_the_plain_audio(eng):
    from smalltts_amd.api import Delivery, SmallTTS
    tts = SmallTTS(engine=eng, seed=0)
    refs, toks, durs = [REF, REF[:3]], [TOKS, TOKS[:4]], [DUR, 0.9]
    plain = tts.synthesize_batch(refs, toks, durs, seeds=[77, 78])
    again = tts.synthesize_batch(refs, toks, durs, seeds=[77, 78], deliver=None)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(plain, again))
    dv = Delivery(8000, "mulaw")
    got = tts.synthesize_batch(refs, toks, durs, seeds=[77, 78], deliver=dv)
    for b, (p, g) in enumerate(zip(plain, got)):
        n = p.shape[1]
        want, cnt = eng.deliver(torch.from_numpy(p[None]).to(eng.device), [n], 8000, "mulaw")
        assert g.dtype == np.uint8 and g.shape == (1, cnt[0]) == (1, n // 3) and n == 3200 * (12, 6)[b]
        assert np.array_equal(g, want[:, :cnt[0]].cpu().numpy())
    with pytest.raises(ValueError, match="trim"):
        tts.synthesize_batch(refs, toks, durs, deliver=dv, trim=True)


@pytest.mark.parametrize("rate,encoding", [(8000, "mulaw"), (48000, "pcm16")])
def test_synthesize_stream_delivers_chunks_whose_concatenation_is_the_whole_delivery(eng, rate, encoding):
    """The whole call is engine.deliver on the concatenated chunks of the plain synthesize_stream (the same seed, so the same decoded
    samples): chunked decode and whole decode differ by fp32 summation order, delivery adds nothing to that."""
    from smalltts_amd.api import Decoder, Delivery, SmallTTS
    tts = SmallTTS(engine=eng, seed=0)
    dv = Delivery(rate, encoding)
    plain = list(tts.synthesize_stream(REF, TOKS, DUR, seed=77))
    again = list(tts.synthesize_stream(REF, TOKS, DUR, seed=77, deliver=None))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(plain, again))
    audio = np.concatenate(plain, axis=1)
    want, cnt = eng.deliver(torch.from_numpy(audio[None]).to(eng.device), [audio.shape[1]], rate, encoding)
    want = want[:, :cnt[0]].cpu().numpy()
    got = list(tts.synthesize_stream(REF, TOKS, DUR, seed=77, deliver=dv))
    bank, up, down, width, klen = eng.deliver_bank(rate)
    sizes = [3200 * c for c in (2, 4, 6)]
    assert [g.shape[1] for g in got] == A.deliver_counts([0, 6400, 19200], sizes, [False, False, True], up, down, width)
    cat = np.concatenate(got, axis=1)
    assert cat.dtype == want.dtype == dv.dtype and cat.shape == want.shape == (1, dv.samples(3200 * N))
    assert np.array_equal(cat, want)
    with pytest.raises(ValueError, match="pcm16"):
        tts.synthesize_stream(REF, TOKS, DUR, deliver=dv, pcm16=True)
    # Decoder.open_stream(deliver=): the same slots behind the codec wrapper, rewound together
    lat = torch.from_numpy(np.concatenate([l for _, l in tts.synthesize_stream(REF, TOKS, DUR, seed=77, return_latents=True)])[None])
    st = Decoder(engine=eng).open_stream(rows=1, deliver=dv)
    a = st.decode(lat[:, :2])
    snap = st.snapshot()
    b = st.decode(lat[:, 2:6])
    c = st.decode(lat[:, 6:], last=True)
    assert np.array_equal(torch.cat([a, b, c], dim=1).numpy(), want)
    st.restore(snap)
    assert torch.equal(st.decode(lat[:, 2:6]), b)
    st.reset()
    assert torch.equal(st.decode(lat[:, :2]), a)


def test_synthesize_long_delivers_the_joined_waveform(eng):
    """One row, behind the join: engine.deliver of the plain call's waveform; segments and words in output samples."""
    from smalltts_amd.api import Delivery, SmallTTS
    tts = SmallTTS(engine=eng, seed=0)
    voice = tts.encode_voice(REF)
    kw = dict(token_lists=[TOKS, TOKS[:4], TOKS[2:]], durations=[0.8, 0.3, 0.5], seed=3, max_batch=2)
    plain, segs, words = tts.synthesize_long(voice, return_segments=True, return_words=True, **kw)
    assert np.array_equal(tts.synthesize_long(voice, deliver=None, **kw).view(np.uint32), plain.view(np.uint32))
    for dv in (Delivery(16000, "pcm16"), Delivery(44100, "alaw"), Delivery(24000, "mulaw")):
        got, dsegs, dwords = tts.synthesize_long(voice, deliver=dv, return_segments=True, return_words=True, **kw)
        S = plain.shape[1]
        want, cnt = eng.deliver(torch.from_numpy(plain[None]).to(eng.device), [S], dv.rate, dv.encoding)
        assert got.dtype == dv.dtype and got.shape == (1, cnt[0]) == (1, dv.samples(S))
        assert np.array_equal(got, want[:, :cnt[0]].cpu().numpy()), dv
        assert dsegs == [(dv.samples(o), dv.samples(o + n) - dv.samples(o), dv.samples(st), g) for o, n, st, g in segs]
        assert dwords == [(i, kind, dv.samples(a), dv.samples(b)) for i, kind, a, b in words]
    with pytest.raises(ValueError, match="pcm16"):
        tts.synthesize_long(voice, deliver=Delivery(8000, "mulaw"), pcm16=True, **kw)


def test_server_answers_at_the_rate_and_encoding_asked_for(eng):
    import threading
    from http.server import ThreadingHTTPServer
    from smalltts_amd import server as S
    from smalltts_amd.api import Delivery, Encoder, SmallTTS
    from tests.test_stream_gpu import _post
    tts, enc = SmallTTS(engine=eng, seed=0), Encoder(engine=eng)
    batcher = S.Batcher(tts, enc, max_batch=8, window_ms=5.0, in_flight=2, num_steps=4)
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), S.make_handler(batcher, tokenizer="chars"))
    httpd.daemon_threads = True
    threading.Thread(target=httpd.serve_forever, kwargs={"poll_interval": 0.02}, daemon=True).start()
    port = httpd.server_address[1]
    sr = 24000
    t = np.arange(int(0.6 * sr)) / sr
    wav = S.encode_wav(0.4 * np.sin(2 * np.pi * 220 * t), sr)
    toks, dur, seed = TOKS, 2.0, 1234
    base = f"duration={dur}&seed={seed}"
    try:
        plain0 = _post(port, wav, toks, base)
        whole = {q: _post(port, wav, toks, f"{base}&{q}") for q in ("rate=8000&encoding=mulaw", "encoding=alaw", "rate=48000")}
        streamed = {q: _post(port, wav, toks, f"{base}&stream=1&{q}") for q in ("rate=8000&encoding=mulaw", "rate=48000&encoding=pcm16")}
        bad = [_post(port, wav, toks, f"{base}&{q}") for q in ("rate=12000", "encoding=f32", "rate=8000&trim=1&level=-20", "rate=abc")]
        plain1 = _post(port, wav, toks, base)
        plain_stream = _post(port, wav, toks, f"{base}&stream=1")
    finally:
        httpd.shutdown()
        httpd.server_close()
        batcher.close()
    assert all(b[0] == 400 for b in bad), [b[0] for b in bad]
    assert plain0[0] == 200 and plain0[2] == plain1[2] and plain0[1]["content-type"] == "audio/wav"   # a plain request is what it was
    assert plain_stream[1]["content-type"] == "audio/L16; rate=24000; channels=1" and plain_stream[1]["x-smtts-pcm"] == "s16le"
    n24 = 3200 * 15
    for q, (tag, rate, bits) in {"rate=8000&encoding=mulaw": (7, 8000, 8), "encoding=alaw": (6, 24000, 8), "rate=48000": (1, 48000, 16)}.items():
        code, heads, body = whole[q]
        assert code == 200 and heads["content-type"] == "audio/wav" and body[:4] == b"RIFF", q
        fmt = body.index(b"fmt ")
        assert tuple(np.frombuffer(body[fmt + 8:fmt + 16], "<u2")[:2]) == (tag, 1) and int(np.frombuffer(body[fmt + 12:fmt + 16], "<u4")[0]) == rate
        y, r = S.decode_wav_bytes(body)
        assert r == rate and y.size == n24 * rate // 24000 and np.isfinite(y).all(), q
    # the streamed bodies are synthesize_stream's bytes under the tuning the server runs
    y, _ = S.decode_wav_bytes(wav)
    lat = enc.encode(torch.from_numpy(np.ascontiguousarray(y[: len(y) // 3200 * 3200]))[None, None])[0].numpy()
    prev = eng.set_tuning("throughput")
    try:
        for q, dv, ctype, pcm in (("rate=8000&encoding=mulaw", Delivery(8000, "mulaw"), "audio/PCMU; rate=8000", "mulaw"),
                                  ("rate=48000&encoding=pcm16", Delivery(48000, "pcm16"), "audio/L16; rate=48000; channels=1", "s16le")):
            code, heads, body = streamed[q]
            assert code == 200 and heads["transfer-encoding"] == "chunked" and heads["content-type"] == ctype and heads["x-smtts-pcm"] == pcm
            want = np.concatenate(list(tts.synthesize_stream(lat, toks, dur, seed=seed, frames=S.frames_for(dur), deliver=dv)), axis=1)
            got = np.frombuffer(body, np.dtype(dv.dtype).newbyteorder("<"))
            assert got.size == want.size == dv.samples(n24) and np.array_equal(got, want.reshape(-1)), q
    finally:
        eng.set_tuning(prev)
