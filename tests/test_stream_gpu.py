"""GPU: the streamed codec decode (include/smalltts_hip.h smtts_codec_decode_stream): carry_frames against its numpy
restatement bit for bit between guard bands, a zero state against the whole decode bit for bit, chunked decodes against the CPU codec
oracle of the WHOLE utterance (which is causal: tests/test_stream_cpu.py) at the bar the whole decode is held to, what is refused, and
the public layers on top (SmallTTS.synthesize_stream, the server's stream=1)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import codec_oracle as CO
from oracle.dit_oracle import to_torch
from smalltts_amd.weights import DEFAULT_CODEC, CodecSpec, codec_decoder_param_specs, decode_state_layout, synth_state_dict
from tests.helpers import stream_ref as SR
from tests.helpers.guarded import Arena
from tests.test_codec_gpu import SNR_BOUND_DB, SPECS, snr_db
from tests.test_precision_gpu import SNR_F16

pytestmark = pytest.mark.gpu
STREAM_SPECS = ("tiny", "odd", "no_bias_no_scale_final_norm")
SEED = 3
FRAMES = 11
SPLITS = ((1,) * 11, (3, 8), (8, 3), (5, 6), (2, 4, 5))


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


_cache = {}


def _setup(name):
    """(engine at bf16x3, spec, latents (3, 11, 64), oracle decode of all 11 frames), built once per spec and left unchanged"""
    if name not in _cache:
        from smalltts_amd.engine import HipEngine
        spec = SPECS[name]
        eng = HipEngine(0, "bf16x3")
        eng.load_synthetic(SEED, parts=("decoder",), codec_spec=spec)
        eng.finalize()
        wd = to_torch(synth_state_dict(codec_decoder_param_specs(spec), SEED))
        lat = torch.randn(3, FRAMES, 64, generator=torch.Generator().manual_seed(5))
        with torch.no_grad():
            ref = CO.decode(wd, lat, spec).numpy()
        _cache[name] = (eng, spec, lat, ref)
    return _cache[name]


def _chunked(eng, lat, split, slots, n_slots=5, zero_before=None):
    """lat (B, sum(split), 64) decoded chunk by chunk on slots `slots` of a fresh pool -> (audio (B, 1, hop * N) on the host, the pool)"""
    state = eng.decode_state(n_slots)
    out, t0 = [], 0
    for k, n in enumerate(split):
        if zero_before == k:
            state.zero_()
        out.append(eng.codec_decode_stream(lat[:, t0:t0 + n], state, slots))
        t0 += n
    assert t0 == lat.shape[1]
    return torch.cat(out, dim=2).cpu().numpy(), state


# ---- 1. carry_frames against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,Cc", [(1, 1, 4), (3, 5, 8), (2, 8, 64), (2, 9, 2048), (3, 40, 32)])
def test_carry_frames_is_the_restatement_bit_for_bit_between_guards(B, T, Cc):
    eng = _setup("tiny")[0]
    n_slots, offset = 7, 48
    stride = (offset + 32 * Cc + 80 + 15) // 16 * 16
    slots = {1: [4], 2: [6, 2], 3: [5, 0, 3]}[B]            # a permutation with gaps
    g = torch.Generator().manual_seed(B * 1000 + T)
    img0 = torch.randn(B, SR.PAD + T, Cc, generator=g)
    pool0 = (torch.arange(n_slots * stride, dtype=torch.int64) * 7 % 251).to(torch.uint8)   # every byte of every slot patterned
    pn = pool0.numpy()
    blocks = np.stack([pn[s * stride + offset:s * stride + offset + 32 * Cc].copy().view(np.float32).reshape(SR.PAD, Cc) for s in slots])
    want_img, want_blocks = SR.carry(img0.numpy(), blocks, T)
    want_pool = pn.copy()
    for b, s in enumerate(slots):
        want_pool[s * stride + offset:s * stride + offset + 32 * Cc] = want_blocks[b].reshape(-1).view(np.uint8)
    ar = Arena("cuda")
    img, pool, tab = ar.put("img", img0), ar.put("pool", pool0), ar.put("slots", torch.tensor(slots, dtype=torch.int64))
    for byte in (0x00, 0xFF):
        img.copy_(img0)
        pool.copy_(pool0)
        ar.paint(byte)
        rc = eng.lib.smtts_test_carry_frames(eng.h, eng._stream(), _p(img), B, T, Cc, _p(pool), stride, offset, _p(tab))
        assert rc == 0, eng.lib.smtts_last_error(eng.h)
        torch.cuda.synchronize()
        ar.assert_clean("smtts_test_carry_frames", (B, T, Cc, byte))
        got_img, got_pool = img.cpu().numpy(), pool.cpu().numpy()
        assert np.array_equal(got_img.view(np.uint32), want_img.view(np.uint32))       # pads = old state, data frames untouched
        assert np.array_equal(got_pool, want_pool)       # the blocks moved on; other slots and the bytes around the block unchanged
        assert np.array_equal(got_img[:, SR.PAD:].view(np.uint32), img0.numpy()[:, SR.PAD:].view(np.uint32))


# ---- 2. a zero state is the whole decode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STREAM_SPECS)
def test_zero_state_is_the_whole_decode_bit_for_bit(name):
    eng, spec, lat, _ = _setup(name)
    B, T = (3, 7) if spec.hop < 1000 else (2, 3)
    x = lat[:B, :T].contiguous()
    whole = eng.codec_decode(x).cpu().numpy()
    slots = [2, 0, 1][:B]
    state = eng.decode_state(3)
    layout, nbytes = decode_state_layout(spec)
    assert tuple(state.shape) == (3, nbytes)
    got = eng.codec_decode_stream(x, state, slots).cpu().numpy()
    assert got.shape == whole.shape == (B, 1, spec.hop * T)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    # the first boundary now holds the last 8 latent frames, zeros in front (T < 8)
    assert layout[0] == ("latent", 64, 0)
    first = state[:, :SR.PAD * 64 * 4].cpu().numpy().view(np.float32).reshape(3, SR.PAD, 64)
    want = np.concatenate([np.zeros((B, SR.PAD - T, 64), np.float32), x.numpy()], axis=1)
    for b, s in enumerate(slots):
        assert np.array_equal(first[s].view(np.uint32), want[b].view(np.uint32))
    if B < 3:
        assert not state[1].any()   # a slot no row names is untouched


# ---- 3. chunked against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STREAM_SPECS)
def test_chunked_decode_is_the_oracle_of_the_whole_utterance(name):
    eng, spec, lat, ref = _setup(name)
    slots = [3, 0, 4]
    for split in SPLITS:
        got, _ = _chunked(eng, lat, split, slots)
        s = snr_db(got, ref)
        print(f"\n[stream] {name} split {split}: {s:.1f} dB")
        assert s >= SNR_BOUND_DB, f"{name} split {split}: {s:.1f} dB"
    # the state is what makes it so: zeroed before the second chunk, the same call misses the bar (the oracle says about 1.6 dB)
    lost, _ = _chunked(eng, lat, (3, 8), slots, zero_before=1)
    s_lost = snr_db(lost, ref)
    print(f"[stream] {name} state lost before chunk 2: {s_lost:.1f} dB")
    assert s_lost < SNR_BOUND_DB
    # ... and a stream does not depend on which slot holds it
    a, _ = _chunked(eng, lat, (2, 4, 5), slots)
    b, _ = _chunked(eng, lat, (2, 4, 5), [1, 2, 0])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 4. the full-size spec ------------------------------------------------------------------------------------------------------------
def test_full_spec_chunked_decode_vs_oracle_and_whole_decode():
    """2 rows x 6 frames in chunks (1, 2, 3).  Measured on an MI355X: see NOTEBOOK 'Streamed decode'."""
    from smalltts_amd.engine import HipEngine
    spec = DEFAULT_CODEC
    layout, nbytes = decode_state_layout(spec)
    eng = HipEngine(0, "bf16x3")
    eng.load_synthetic(9, parts=("decoder",), codec_spec=spec)
    eng.finalize()
    assert eng.decode_state_bytes == nbytes == 849920 and len(layout) == 34
    wd = to_torch(synth_state_dict(codec_decoder_param_specs(spec), 9))
    lat = torch.randn(2, 6, 64, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = CO.decode(wd, lat, spec).numpy()
    for prec, bar in (("bf16x3", SNR_BOUND_DB), ("f16", SNR_F16)):
        eng.set_precision(prec)
        whole = eng.codec_decode(lat).cpu().numpy()
        got, _ = _chunked(eng, lat, (1, 2, 3), [1, 0], n_slots=2)
        s_whole, s_chunk, s_between = snr_db(whole, ref), snr_db(got, ref), snr_db(got, whole)
        print(f"\n[stream] full spec {prec}: chunked {s_chunk:.1f} dB, whole {s_whole:.1f} dB vs the oracle; chunked vs whole {s_between:.1f} dB")
        assert s_chunk >= s_whole - 1.0, f"{prec}: chunked {s_chunk:.1f} dB, whole {s_whole:.1f} dB"
        assert s_chunk > bar, f"{prec}: chunked {s_chunk:.1f} dB"


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refused_calls_enqueue_nothing():
    eng, spec, lat, ref = _setup("tiny")
    from smalltts_amd.engine import HipEngine
    B, T = 3, 4
    x = lat[:, :T].contiguous().cuda()
    sb = eng.decode_state_bytes
    need = int(eng.lib.smtts_decode_stream_workspace_bytes(eng.h, B, T))
    assert need > 0 and need == int(eng.lib.smtts_decode_workspace_bytes(eng.h, B, T))
    assert eng.lib.smtts_decode_stream_workspace_bytes(eng.h, 0, T) == 0 and eng.lib.smtts_decode_stream_workspace_bytes(eng.h, B, 0) == 0
    raw = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    a0 = (-raw.data_ptr()) % 256
    ws = raw[a0:a0 + need]
    praw = torch.empty(4 * sb + 64, dtype=torch.uint8, device="cuda")
    p0 = (-praw.data_ptr()) % 16
    mark = (torch.arange(praw.numel(), device="cuda") % 13).to(torch.uint8)
    praw.copy_(mark)
    pool = praw[p0:p0 + 4 * sb]
    tab = torch.tensor([3, 0, 2], dtype=torch.int64, device="cuda")
    audio = torch.full((B, 1, spec.hop * T), 7.0, device="cuda")

    def call(h=None, lat_=x, B_=B, T_=T, pool_=pool, n_=4, tab_=tab, ws_=ws, wsb=need):
        return eng.lib.smtts_codec_decode_stream(eng.h if h is None else h, eng._stream(), _p(lat_), B_, T_, _p(pool_), n_, _p(tab_),
                                                 _p(audio), _p(ws_), wsb)
    bare = HipEngine(0, "bf16x3")   # no decoder
    assert bare.lib.smtts_decode_state_bytes(bare.h) == 0
    cases = {"workspace too small": dict(wsb=need - 1), "workspace misaligned": dict(ws_=raw[a0 + 16:a0 + 16 + need]),
             "pool misaligned": dict(pool_=praw[p0 + 4:p0 + 4 + 3 * sb], n_=3), "no slots": dict(n_=0), "B = 0": dict(B_=0),
             "T = 0": dict(T_=0), "null table": dict(tab_=None), "no decoder": dict(h=bare.h)}
    for what, kw in cases.items():
        assert call(**kw) == 1, what
        msg = (bare if what == "no decoder" else eng).lib.smtts_last_error(kw.get("h", eng.h)).decode()
        assert "codec_decode_stream" in msg, (what, msg)
    torch.cuda.synchronize()
    assert bool((audio == 7.0).all()) and torch.equal(praw, mark)   # nothing ran: not a sample written, not a state byte moved
    # the Python wrapper sees the table on the host: duplicate and out-of-range slots never reach the device
    state = eng.decode_state(4)
    for bad in ([1, 1, 2], [0, 1, 4], [0, 1], [-1, 0, 1]):
        with pytest.raises(ValueError, match="distinct slots"):
            eng.codec_decode_stream(x, state, bad)
    with pytest.raises(ValueError, match="state must be"):
        eng.codec_decode_stream(x, state[:, :-256], [0, 1, 2])
    assert not state.any()
    assert call() == 0   # and the call the refusals were cut from goes through
    torch.cuda.synchronize()
    assert bool((audio != 7.0).any())


@pytest.mark.parametrize("name", STREAM_SPECS)
def test_unfused_paths_carry_the_state_too(name):
    """smtts_test_set_fused_ffn(h, 0): the two-launch mixer reads pad frames of the NORMALISED image; the streamed decode normalises the
    carried frames as well instead of refusing the configuration, so it meets the bar of the fused paths."""
    eng, spec, lat, ref = _setup(name)
    eng.lib.smtts_test_set_fused_ffn(eng.h, 0)
    try:
        for split in ((3, 8), (2, 4, 5)):
            got, _ = _chunked(eng, lat, split, [3, 0, 4])
            s = snr_db(got, ref)
            print(f"\n[stream] {name} unfused, split {split}: {s:.1f} dB")
            assert s >= SNR_BOUND_DB, f"{name} split {split}: {s:.1f} dB"
    finally:
        eng.lib.smtts_test_set_fused_ffn(eng.h, 1)


# ---- 6. SmallTTS.synthesize_stream ----------------------------------------------------------------------------------------------------
API_SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))   # hop 3200 (what the API assumes), tiny channels
API_SEED = 11


@pytest.fixture(scope="module")
def api_eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(API_SEED, parts=("dit", "decoder", "encoder"), codec_spec=API_SPEC)
    e.finalize()
    return e


def test_synthesize_stream_is_synthesize_batch_in_chunks(api_eng):
    """The DiT at the shape of tests/golden/case_small.npz: 12 frames, a reference of 5 frames, 7 tokens."""
    from smalltts_amd.api import SmallTTS, stream_chunks
    eng = api_eng
    tts = SmallTTS(engine=eng, seed=0)
    ref = torch.randn(5, 64, generator=torch.Generator().manual_seed(0)).numpy()
    toks, dur, N = [3, 17, 42, 99, 150, 7, 8], 1.7, 12
    want_a, want_l = tts.synthesize_batch([ref], [toks], [dur], seeds=[77], return_latents=True)
    got = list(tts.synthesize_stream(ref, toks, dur, seed=77, return_latents=True))
    assert [c.shape[1] for c, _ in got] == [3200 * n for n in stream_chunks(N)] == [6400, 12800, 19200]
    lat = np.concatenate([l for _, l in got])
    audio = np.concatenate([c for c, _ in got], axis=1)
    assert np.array_equal(lat.view(np.uint32), want_l[0].view(np.uint32))      # the sampler ran exactly as synthesize_batch runs it
    assert audio.shape == want_a[0].shape == (1, 3200 * N) and audio.dtype == np.float32
    # same kernels on the same values, other chunk sizes: fp32 summation order at most (test 4 measures bit-identity at full size)
    s = snr_db(audio, want_a[0])
    print(f"\n[stream] synthesize_stream vs synthesize_batch: {s:.1f} dB")
    assert s > 80.0
    # pcm16=True: the same chunks through engine.pcm16
    pcm = list(tts.synthesize_stream(ref, toks, dur, seed=77, pcm16=True))
    for p, (c, _) in zip(pcm, got):
        assert p.dtype == np.int16 and np.array_equal(p, eng.pcm16(c).cpu().numpy())
    # an utterance shorter than the first chunk size is one chunk; a voice instead of the reference gives the same stream
    one = list(tts.synthesize_stream(ref, toks, None, frames=1, seed=5))
    assert len(one) == 1 and one[0].shape == (1, 3200)
    voice = tts.encode_voice(ref)
    via_voice = np.concatenate(list(tts.synthesize_stream(None, toks, dur, seed=77, voice=voice)), axis=1)
    assert snr_db(via_voice, audio) > 80.0
    with pytest.raises(ValueError, match="chunk_frames"):
        tts.synthesize_stream(ref, toks, dur, chunk_frames=())
    # Decoder.open_stream: the same state behind the codec wrapper, with reset and rewind
    from smalltts_amd.api import Decoder
    st = Decoder(engine=eng).open_stream(rows=1)
    x = torch.from_numpy(want_l[0][None])
    a = st.decode(x[:, :5])
    snap = st.snapshot()
    b = st.decode(x[:, 5:])
    assert snr_db(torch.cat([a, b], dim=2).numpy()[0], want_a[0]) > 80.0
    st.restore(snap)
    assert torch.equal(st.decode(x[:, 5:]), b)
    st.reset()
    assert torch.equal(st.decode(x[:, :5]), a)


# ---- 7. the server --------------------------------------------------------------------------------------------------------------------
def _post(port, wav, tokens, query):
    import http.client
    bd = "----t"
    body = (f"--{bd}\r\nContent-Disposition: form-data; name=\"audio\"; filename=\"r.wav\"\r\n\r\n".encode() + wav + b"\r\n"
            + f"--{bd}\r\nContent-Disposition: form-data; name=\"tokens\"\r\n\r\n{tokens}\r\n--{bd}--\r\n".encode())
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", f"/synthesize?{query}", body=body, headers={"content-type": f"multipart/form-data; boundary={bd}"})
    r = c.getresponse()
    data = r.read()            # http.client removes the chunk framing
    heads = {k.lower(): v for k, v in r.getheaders()}
    c.close()
    return r.status, heads, data


def test_server_streams_the_pcm16_of_synthesize_stream(api_eng):
    import threading
    from http.server import ThreadingHTTPServer
    from smalltts_amd import server as S
    from smalltts_amd.api import Encoder, SmallTTS
    eng = api_eng
    tts, enc = SmallTTS(engine=eng, seed=0), Encoder(engine=eng)
    batcher = S.Batcher(tts, enc, max_batch=8, window_ms=5.0, in_flight=2, num_steps=4)
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), S.make_handler(batcher, tokenizer="chars"))
    httpd.daemon_threads = True
    threading.Thread(target=httpd.serve_forever, kwargs={"poll_interval": 0.02}, daemon=True).start()
    port = httpd.server_address[1]
    sr = 24000
    t = np.arange(int(0.6 * sr)) / sr
    wav = S.encode_wav(0.4 * np.sin(2 * np.pi * 220 * t), sr)
    toks, dur, seed = [3, 17, 42, 99, 150, 7, 8], 2.0, 1234          # 2 s = 15 frames exactly, rounded up or down
    try:
        plain0 = _post(port, wav, toks, f"duration={dur}&seed={seed}")
        code, heads, body = _post(port, wav, toks, f"duration={dur}&seed={seed}&stream=1")
        bad = [_post(port, wav, toks, f"duration={dur}&seed={seed}&stream=1&{q}") for q in ("trim=1", "align=1")]
        odd = _post(port, wav, toks, f"duration={dur}&stream=2")
        plain1 = _post(port, wav, toks, f"duration={dur}&seed={seed}")
    finally:
        httpd.shutdown()
        httpd.server_close()
        batcher.close()
    assert code == 200 and heads["transfer-encoding"] == "chunked" and heads["content-type"] == "audio/L16; rate=24000; channels=1"
    assert all(b[0] == 400 and b"stream" in b[2] for b in bad) and odd[0] == 400
    assert plain0[0] == 200 and plain0[2][:4] == b"RIFF" and plain0[2] == plain1[2]       # a plain request is what it was, before and after
    assert "transfer-encoding" not in plain0[1] and plain0[1]["content-type"] == "audio/wav"
    assert batcher.stats["streamed"] == 1
    # the same request through the Python API under the tuning the server runs (the dispatcher restored the engine's own on close)
    y, _ = S.decode_wav_bytes(wav)
    lat = enc.encode(torch.from_numpy(np.ascontiguousarray(y[: len(y) // 3200 * 3200]))[None, None])[0].numpy()
    prev = eng.set_tuning("throughput")
    try:
        want = np.concatenate(list(tts.synthesize_stream(lat, toks, dur, seed=seed, pcm16=True, frames=S.frames_for(dur))), axis=1)
    finally:
        eng.set_tuning(prev)
    got = np.frombuffer(body, "<i2")
    assert got.size == want.size == 3200 * 15
    assert np.array_equal(got, want.reshape(-1))


def test_interactive_cli_stream_prints_the_time_to_the_first_chunk(tmp_path, capsys):
    """interactive.py --stream: the same utterance, decoded in chunks; the report names the first chunk."""
    from smalltts_amd import api
    from smalltts_amd.audio import read_wav
    from smalltts_amd.scripts import interactive
    args = ["--weights", "synthetic:3", "--seed", "0", "--tokenizer", "chars", "--outdir", str(tmp_path)]
    n = interactive.main(args + ["--stream"], lines=["hello there"])
    out = capsys.readouterr().out
    streamed, rate = read_wav(str(tmp_path / "interactive_000.wav"))
    assert n == 1 and "first chunk" in out and "x rt" in out
    assert rate == 24000 and streamed.size % 3200 == 0 and streamed.size > 0 and np.isfinite(streamed).all()
    n = interactive.main(args, lines=["hello there"])                       # without the flag: no such figure, the same length
    out = capsys.readouterr().out
    api._ENGINES.clear()
    whole, _ = read_wav(str(tmp_path / "interactive_000.wav"))
    assert n == 1 and "first chunk" not in out and whole.size == streamed.size
