"""GPU: the endpoint kernels (frame_energy, endpoint_decide, the segment stitch) against the numpy restatement of their definition
(tests/helpers/endpoint_ref.py), and the surface on top: synthesize_long(trim=), synthesize_batch(trim=), encode_voice_wav(trim=),
the server's trim=1.  The engine is built like tests/test_longform_gpu.py's (split-bf16, seed 11, the tiny codec).

Bounds (none of them measured): a frame's mean power is W rounded products, a W-term fp32 sum of non-negative terms in some order and
one division, so its relative error against float64 is at most 2 W 2^-24 (2.9e-5 at W = 240); the gain is an F-term sum of that
kind, a division, a square root and another division: (F + 4) 2^-24.  Everything else is exact."""
import ctypes as C
import http.client
import threading

import numpy as np
import pytest
import torch

from smalltts_amd import server as S
from smalltts_amd.api import HOP_SIZE, Endpointing, fade_table, plan_long, plan_packed
from smalltts_amd.weights import CodecSpec
from tests.helpers import endpoint_ref as R
from tests.helpers.longform_ref import STITCH_CASES, pcm16_numpy, stitch_case

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
U = 2.0 ** -24
SHARP = dict(rel_db=3, min_run=1, floor_dbfs=-200)      # only frames within 3 dB of the loudest are active: any audio that is not flat is cut


class Params:
    """A raw kernel parameter set where the tests do not go through Endpointing."""

    def __init__(self, **kw):
        self.p = R.params(**kw)

    def kernel_params(self):
        return self.p


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(SEED, parts=("dit", "decoder", "encoder"), codec_spec=SPEC)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def tts(eng):
    from smalltts_amd.api import SmallTTS
    return SmallTTS(engine=eng, seed=1)


@pytest.fixture(scope="module")
def voice(tts):
    return tts.encode_voice(np.random.default_rng(0).standard_normal((9, 64)).astype(np.float32))


def run_endpoints(eng, rows, ep, stride=None):
    """rows [(x, n)] as one padded batch with NaN behind every row -> host (seg (B,2), gain (B), [e_b], [pk_b]) cut to each row's frames."""
    audio, lens = R.pad_batch(rows, np.nan, stride)
    seg, gain, e, pk = eng.endpoints(torch.from_numpy(audio).to(eng.device), None, ep, lens=lens, return_peaks=True)
    torch.cuda.synchronize()
    W = int(ep.kernel_params()["W"])
    e, pk = e.cpu().numpy(), pk.cpu().numpy()
    Fs = [(n + W - 1) // W for n in lens]
    return seg.cpu().numpy(), gain.cpu().numpy(), [e[b, :F].copy() for b, F in enumerate(Fs)], [pk[b, :F].copy() for b, F in enumerate(Fs)]


def check_rows(rows, ep, seg, gain, es, pks, from_samples: bool):
    """Checks 5 - 8 on one batch; -> the reference's (start, n, gain) per row from the device's own e."""
    p = ep.kernel_params()
    W = int(p["W"])
    refs = []
    for b, (x, n) in enumerate(rows):
        e64, pk64 = R.frame_energy_ref(x, n, W, np.float64)
        e, pk = es[b], pks[b]
        assert e.shape == e64.shape and np.isfinite(e).all() and np.isfinite(pk).all(), b          # nothing behind len[b] was read
        assert np.array_equal(e == 0, e64 == 0), b
        nz = e64 > 0
        rel = np.abs(e[nz].astype(np.float64) - e64[nz]) / e64[nz]
        assert rel.size == 0 or rel.max() <= 2 * W * U, (b, rel.max())
        assert (pk.max() if pk.size else 0.0) == (np.abs(x[:n]).max() if n else 0.0), b
        own = R.decide_ref(e, pk, n, p)                                                             # fp32, from the returned e
        assert (int(seg[b, 0]), int(seg[b, 1])) == own[:2], (b, seg[b], own)
        if from_samples:
            assert (int(seg[b, 0]), int(seg[b, 1])) == R.decide_ref(e64, pk64, n, p)[:2], (b, seg[b])
        g64 = R.decide_ref(e.astype(np.float64), pk, n, p)[2]
        if float(p["target_rms"]) == 0.0 or seg[b, 1] == 0:
            assert gain[b] == 1.0 and g64 == 1.0, (b, gain[b])
        else:
            assert abs(float(gain[b]) - g64) <= (len(e) + 4) * U * g64, (b, gain[b], g64)
        refs.append((own[0], own[1], g64))
    return refs


@pytest.mark.parametrize("seed", R.CASE_SEEDS)
def test_crafted_rows_energies_decisions_and_gain(eng, seed):
    rows = R.endpoint_case(seed)
    ep = Params()
    seg, gain, es, pks = run_endpoints(eng, rows, ep)
    check_rows(rows, ep, seg, gain, es, pks, from_samples=True)
    assert (gain == 1.0).all()                                      # target_rms = 0
    lvl = Params(target_rms=np.float32(0.25), max_gain=np.float32(2.0))
    seg2, gain2, es2, pks2 = run_endpoints(eng, rows, lvl)
    check_rows(rows, lvl, seg2, gain2, es2, pks2, from_samples=True)
    assert np.array_equal(seg, seg2) and all(np.array_equal(a, b) for a, b in zip(es, es2))
    # twice the same launch, an odd row stride (the scalar load path), every row alone at B = 1: the same bits
    for other in (run_endpoints(eng, rows, lvl), run_endpoints(eng, rows, lvl, stride=max(n for _, n in rows) + 1)):
        assert np.array_equal(other[0], seg2) and np.array_equal(other[1], gain2)
        assert all(np.array_equal(a, b) for a, b in zip(other[2], es2)) and all(np.array_equal(a, b) for a, b in zip(other[3], pks2))
    for b in (0, 3, 5, 6, 7):
        one = run_endpoints(eng, [rows[b]], lvl)
        assert np.array_equal(one[0][0], seg2[b]) and one[1][0] == gain2[b] and np.array_equal(one[2][0], es2[b]), b


def test_both_gain_clamps_are_hit(eng):
    lvl = Params(target_rms=np.float32(0.25), max_gain=np.float32(2.0))
    p = lvl.kernel_params()
    capped = peaked = free = 0
    for seed in R.CASE_SEEDS[:6]:
        rows = R.endpoint_case(seed)
        seg, gain, es, pks = run_endpoints(eng, rows, lvl)
        for b in range(len(rows)):
            if seg[b, 1] == 0:
                continue
            capped += gain[b] == p["max_gain"]
            peaked += gain[b] == np.float32(p["peak_limit"] / pks[b].max()) and gain[b] < p["max_gain"]
    soft = Params(target_rms=np.float32(0.01))
    seg, gain, es, pks = run_endpoints(eng, R.endpoint_case(0), soft)
    free = int(((gain != 1.0) & (gain < 1.0)).sum())
    print(f"rows whose gain stopped at max_gain: {capped}, at the peak limit: {peaked}, unclamped (target -40 dBFS): {free}")
    assert capped >= 1 and peaked >= 1 and free >= 1


def test_other_frame_sizes_and_min_run(eng):
    """W = 16 (the smallest), 304, 4096 (the largest), min_run 1 and 16, rows longer than one sweep of the decision kernel's 256 threads."""
    g = np.random.default_rng(3)
    x = np.zeros(100000, np.float32)
    x[30000:70000] = (g.standard_normal(40000) * 0.1).astype(np.float32)
    x[5000:5000 + 600] = (g.standard_normal(600) * 0.1).astype(np.float32)
    rows = [(x, 100000), (x[:61111].copy(), 61111), (x[29000:].copy(), 71000), (np.zeros(1, np.float32), 0)]
    for W, min_run in ((16, 1), (16, 16), (304, 1), (304, 3), (4096, 1), (4096, 2)):
        ep = Params(W=W, min_run=min_run, lead=100, tail=100, target_rms=np.float32(0.05))
        seg, gain, es, pks = run_endpoints(eng, rows, ep)
        refs = check_rows(rows, ep, seg, gain, es, pks, from_samples=False)
        assert refs[0][1] > 0 and refs[3][:2] == (0, 0)


def test_bad_arguments_are_refused(eng):
    a = torch.zeros(2, 1, 6400, device=eng.device)
    for kw in (dict(W=242), dict(W=12), dict(W=8192), dict(min_run=0), dict(min_run=17), dict(lead=-1)):
        with pytest.raises(ValueError):
            eng.endpoints(a, [1, 2], Params(**kw))
    with pytest.raises(ValueError):
        eng.endpoints(a, [1, 3], Params())                    # longer than the row
    with pytest.raises(ValueError):
        eng.endpoints(a[:, :, ::2], [1, 1], Params())
    seg, gain, e = eng.endpoints(a, [1, 2], Params())
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    lens = torch.tensor([3200, 6400], dtype=torch.int64, device=eng.device)
    call = lambda W, min_run, lead: eng.lib.smtts_endpoints(eng.h, eng._stream(), p(a), 2, 6400, p(lens), W, 1e-4, 1e-8, min_run, lead, 0, 0.0,
                                                            0.9, 10.0, p(e), p(e), p(seg), p(gain))
    assert call(242, 3, 0) != 0 and b"W" in eng.lib.smtts_last_error(eng.h)
    assert call(240, 0, 0) != 0 and call(240, 3, -1) != 0 and call(240, 17, 0) != 0
    out = torch.zeros(10, device=eng.device)
    with pytest.raises(ValueError):
        eng.stitch_seg(a, seg[:1], None, [0, 0], None, out)
    with pytest.raises(ValueError):
        eng.stitch_seg(a, seg, gain.double(), [0, 0], None, out)
    with pytest.raises(ValueError):
        eng.stitch_seg(a, seg, None, [0, 11], None, out)


@pytest.mark.parametrize("case", range(len(STITCH_CASES)))
@pytest.mark.parametrize("pcm16", [False, True])
def test_stitch_seg_bit_for_bit(eng, case, pcm16):
    hop, batches, F, gap = STITCH_CASES[case]
    rows, fade, S = stitch_case(hop, batches, F, gap, seed=case)
    g = np.random.default_rng(100 + case)
    dt = np.int16 if pcm16 else np.float32
    tdt = torch.int16 if pcm16 else torch.float32
    fade_d = torch.from_numpy(fade).to(eng.device) if F else None
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    # (a) the whole rows without gain: smtts_stitch's bits
    want = torch.zeros(S, dtype=tdt, device=eng.device)
    got = torch.zeros(S, dtype=tdt, device=eng.device)
    for audio, lens, offs in rows:
        a = torch.from_numpy(audio).to(eng.device)
        tab = torch.tensor([lens, offs], dtype=torch.int64, device=eng.device)
        rc = eng.lib.smtts_stitch(eng.h, eng._stream(), p(a), a.shape[0], a.shape[-1], p(tab[0]), p(tab[1]), p(fade_d), F, p(want), S, int(pcm16))
        assert rc == 0, eng.lib.smtts_last_error(eng.h)
        seg = torch.tensor([(0, n) for n in lens], dtype=torch.int64, device=eng.device)
        eng.stitch_seg(a, seg, None, offs, fade_d, got)
    assert torch.equal(got, want) and bool(got.any())
    # (b) random windows (odd starts, empty ones, windows shorter than two fades) with and without gain, packed `gap` apart
    for with_gain in (False, True):
        segs, pos, plan = [], 0, []
        for audio, lens, _ in rows:
            sg = []
            for n in lens:
                s = int(g.integers(0, n))
                sg.append((s, int(g.integers(0, n - s + 1)) if g.random() > 0.15 else 0))
            segs.append(sg)
            plan.append([])
            for _, m in sg:
                plan[-1].append(pos)
                pos += m + gap
        total = max(pos, 1)
        want = np.zeros(total, dt)
        got = torch.zeros(total, dtype=tdt, device=eng.device)
        for (audio, lens, _), sg, offs in zip(rows, segs, plan):
            gain = g.uniform(0.2, 3.0, len(lens)).astype(np.float32) if with_gain else None
            R.stitch_seg_numpy(want, audio, sg, gain, offs, fade)
            eng.stitch_seg(torch.from_numpy(audio).to(eng.device), torch.tensor(sg, dtype=torch.int64, device=eng.device),
                           None if gain is None else torch.from_numpy(gain).to(eng.device), offs, fade_d, got)
        got = got.cpu().numpy()
        assert np.array_equal(got, want), (case, pcm16, with_gain, int((got != want).sum()))


def _long_kw():
    g = np.random.default_rng(12)
    durs = [1.0, 2.2, 1.5, 0.7, 3.0, 1.2, 2.0, 0.5, 1.8, 2.6, 0.9]
    toks = [[int(t) for t in g.integers(1, 198, size=int(g.integers(3, 20)))] for _ in durs]
    return dict(token_lists=toks, durations=durs, seed=3, max_batch=4, in_flight=3), [max(1, int(d * 7.5)) for d in durs]


def test_synthesize_long_without_trim_is_untouched(tts, voice):
    kw, ns = _long_kw()
    a = tts.synthesize_long(voice, **kw)
    b = tts.synthesize_long(voice, trim=None, **kw)
    c, segs = tts.synthesize_long(voice, trim=False, return_segments=True, **kw)
    assert np.array_equal(a, b) and np.array_equal(a, c) and a.any()
    _, offsets, S = plan_long(ns, 4, 120.0)
    assert segs == [(offsets[i], HOP_SIZE * ns[i], 0, 1.0) for i in range(len(ns))] and a.shape == (1, S)


def _pieces_batches(full, ns, offsets, group=4):
    """The untrimmed join at fade 0 holds every piece as a pure copy at plan_long's offset: padded batches of them, NaN behind."""
    rows = [(full[0, o:o + HOP_SIZE * n].copy(), HOP_SIZE * n) for o, n in zip(offsets, ns)]
    return [rows[i:i + group] for i in range(0, len(rows), group)]


@pytest.mark.parametrize("fade_ms", [0.0, 5.0])
def test_synthesize_long_trimmed_equals_the_numpy_composition(eng, tts, voice, fade_ms):
    kw, ns = _long_kw()
    ep = Endpointing(level_dbfs=-20, **SHARP)
    full = tts.synthesize_long(voice, trim=None, fade_ms=0.0, **kw)
    assert full.any() and np.isfinite(full).all()
    _, offsets, _ = plan_long(ns, 4, 120.0)
    out, segs = tts.synthesize_long(voice, trim=ep, fade_ms=fade_ms, return_segments=True, **kw)
    pcm = tts.synthesize_long(voice, trim=ep, fade_ms=fade_ms, pcm16=True, **kw)
    assert len(segs) == len(ns)
    table = []
    for rows in _pieces_batches(full, ns, offsets):                 # engine.endpoints on the pieces reproduces the table exactly
        seg, gain, es, pks = run_endpoints(eng, rows, ep)
        check_rows(rows, ep, seg, gain, es, pks, from_samples=False)
        table += [(int(seg[b, 0]), int(seg[b, 1]), float(gain[b])) for b in range(len(rows))]
    assert [(s[2], s[1], s[3]) for s in segs] == table, (segs, table)
    lens = [HOP_SIZE * n for n in ns]
    print("pieces (len, start, n, gain):", [(l, *t) for l, t in zip(lens, table)])
    assert any(t[1] < l for t, l in zip(table, lens)), "nothing was trimmed: the comparison shows nothing"
    pk_offs, S = plan_packed([t[1] for t in table], 120.0)
    assert out.shape == pcm.shape == (1, S) and [s[0] for s in segs] == pk_offs
    want = np.zeros(S, np.float32)
    audio = np.zeros((len(ns), 1, max(lens)), np.float32)
    for i, (o, l) in enumerate(zip(offsets, lens)):
        audio[i, 0, :l] = full[0, o:o + l]
    R.stitch_seg_numpy(want, audio, [t[:2] for t in table], np.asarray([t[2] for t in table], np.float32), pk_offs, fade_table(fade_ms))
    assert np.array_equal(out[0], want)
    wpcm = np.zeros(S, np.int16)
    R.stitch_seg_numpy(wpcm, audio, [t[:2] for t in table], np.asarray([t[2] for t in table], np.float32), pk_offs, fade_table(fade_ms))
    assert pcm.dtype == np.int16 and np.array_equal(pcm[0], wpcm)
    gap = round(120.0 * 24)
    live = [i for i, t in enumerate(table) if t[1]]
    for i in live[:-1]:                                             # the gaps are silence, and exactly gap_ms wide
        lo = pk_offs[i] + table[i][1]
        assert not out[0, lo:lo + gap].any()
    # without a level the samples are pure copies of the windows
    plain, psegs = tts.synthesize_long(voice, trim=Endpointing(**SHARP), fade_ms=0.0, return_segments=True, **kw)
    assert [s[:3] for s in psegs] == [s[:3] for s in segs]          # neither the fade nor the level moves a window
    for (o, n, s, gain), po, l in zip(psegs, offsets, lens):
        assert gain == 1.0 and np.array_equal(plain[0, o:o + n], full[0, po + s:po + s + n])


def test_synthesize_long_endpoints_of_a_decoded_batch(eng, tts, voice):
    """Check 6 on whatever the synthetic model decodes, default Endpointing and a levelled one, straight on the device batch."""
    toks = [[1, 2, 3, 4], [10, 20, 30, 40, 50, 60], [7] * 9]
    ns = [7, 16, 11]
    audio = tts.synthesize_batch(None, toks, None, frames=ns, voices=[voice] * 3, seeds=[5, 6, 7], _defer=True).audio
    host = audio.cpu().numpy()
    rows = [(host[b, 0].copy(), HOP_SIZE * ns[b]) for b in range(3)]
    for ep in (Endpointing(), Endpointing(level_dbfs=-23), Endpointing(level_dbfs=-20, **SHARP)):
        seg, gain, e, pk = eng.endpoints(audio, ns, ep, return_peaks=True)
        seg2, gain2, es, pks = run_endpoints(eng, rows, ep)
        assert np.array_equal(seg.cpu().numpy(), seg2) and np.array_equal(gain.cpu().numpy(), gain2)   # the padding is not read
        check_rows(rows, ep, seg2, gain2, es, pks, from_samples=False)


def test_synthesize_batch_trim_returns_the_windows(eng, tts, voice):
    toks = [[1, 2, 3, 4], [10, 20, 30, 40, 50, 60], [7] * 9]
    durs = [1.0, 2.2, 1.5]
    kw = dict(voices=[voice] * 3, seeds=[5, 6, 7])
    full = tts.synthesize_batch(None, toks, durs, **kw)
    assert tts.synthesize_batch(None, toks, durs, trim=None, **kw)[0].shape == full[0].shape
    for ep in (Endpointing(**SHARP), Endpointing(level_dbfs=-20, **SHARP), True):
        got, lat = tts.synthesize_batch(None, toks, durs, trim=ep, return_latents=True, **kw)
        ep_ = Endpointing() if ep is True else ep
        cut = 0
        for b in range(3):
            rows = [(full[b][0].copy(), full[b].shape[1])]
            seg, gain, _, _ = run_endpoints(eng, rows, ep_)
            s, n = int(seg[0, 0]), int(seg[0, 1])
            want = full[b][:, s:s + n]
            if ep_.level_dbfs is not None:
                want = want * np.float32(gain[0])
            assert got[b].shape == (1, n) and got[b].dtype == np.float32 and np.array_equal(got[b], want), b
            cut += n < full[b].shape[1]
        assert lat[1].shape == (16, 64)
        print(f"{ep_!r}: {cut} of 3 rows cut")
    with pytest.raises(TypeError):
        tts.synthesize_batch(None, toks, durs, trim="yes", **kw)


def test_encode_voice_wav_trim(eng, tts):
    g = np.random.default_rng(4)
    t = np.arange(int(1.1 * 24000)) / 24000.0
    clip = (0.4 * np.sin(2 * np.pi * 220 * t) * (1 + 0.3 * np.sin(2 * np.pi * 3 * t)) + 0.01 * g.standard_normal(t.size)).astype(np.float32)
    padded = np.concatenate([np.zeros(12000, np.float32), clip, np.zeros(12000, np.float32)])
    ep = Endpointing()
    seg, _, _, _ = run_endpoints(eng, [(padded, padded.size)], ep)
    s, n = int(seg[0, 0]), int(seg[0, 1])
    assert s == 12000 - 720 - 12000 % 240 and 0 < n < padded.size                 # the window engine.endpoints reports ...
    n_cut = max(HOP_SIZE, n // HOP_SIZE * HOP_SIZE)                                # ... rounded down to whole hops
    by_hand = tts.encode_voice_wav(padded[s:s + n_cut], 24000)
    v = tts.encode_voice_wav(padded, 24000, trim=True)
    whole = tts.encode_voice_wav(padded, 24000)
    assert v.R == n_cut // HOP_SIZE < whole.R
    assert torch.equal(v.k_ref, by_hand.k_ref) and torch.equal(v.v_ref, by_hand.v_ref)
    assert torch.equal(tts.encode_voice_wav(padded, 24000, trim=ep).k_ref, v.k_ref)
    with pytest.raises(ValueError):
        tts.encode_voice_wav(np.zeros(30000, np.float32), 24000, trim=True)


def _post(port, wav, tokens, query):
    bd = "----t"
    body = (f"--{bd}\r\nContent-Disposition: form-data; name=\"audio\"; filename=\"r.wav\"\r\n\r\n".encode() + wav + b"\r\n"
            + f"--{bd}\r\nContent-Disposition: form-data; name=\"tokens\"\r\n\r\n{tokens}\r\n--{bd}--\r\n".encode())
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=120)
    c.request("POST", "/synthesize?" + query, body=body, headers={"content-type": f"multipart/form-data; boundary={bd}"})
    r = c.getresponse()
    data = r.read()
    c.close()
    return r.status, {k.lower(): v for k, v in r.getheaders()}, data


def test_server_trim(eng, tts):
    """One request at a time (each rides alone, so the same seed gives the same bits): trim=1 answers the window of the untrimmed
    answer that its headers name; trim=0 and no parameter answer the same bytes without the headers.  Then the batcher directly,
    where the futures carry fp32: a sharp Endpointing really cuts, a level multiplies by the device's gain."""
    from http.server import ThreadingHTTPServer
    from smalltts_amd.api import Encoder
    batcher = S.Batcher(tts, Encoder(engine=eng), max_batch=8, window_ms=1.0, in_flight=2, num_steps=4)
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), S.make_handler(batcher, tokenizer="chars"))
    httpd.daemon_threads = True
    threading.Thread(target=httpd.serve_forever, kwargs={"poll_interval": 0.02}, daemon=True).start()
    port = httpd.server_address[1]
    t = np.arange(int(0.7 * 24000)) / 24000.0
    ref = (0.4 * np.sin(2 * np.pi * 260 * t)).astype(np.float32)
    wav = S.encode_wav(ref, 24000)
    try:
        st0, h0, plain = _post(port, wav, "5,9,14,33,41", "duration=1.3&seed=77")
        st1, h1, off = _post(port, wav, "5,9,14,33,41", "duration=1.3&seed=77&trim=0")
        st2, h2, cut = _post(port, wav, "5,9,14,33,41", "duration=1.3&seed=77&trim=1")
        st3, _, msg = _post(port, wav, "5,9,14,33,41", "duration=1.3&seed=77&trim=1&level=7")
        y_ref, sr = S.decode_wav_bytes(wav)
        futs = [batcher.submit(S.Request(y_ref, sr, [5, 9, 14, 33, 41], 1.3, 77, ep)).result(timeout=120)
                for ep in (None, Endpointing(**SHARP), Endpointing(level_dbfs=-20, **SHARP))]
    finally:
        httpd.shutdown()
        httpd.server_close()
        batcher.close()
    assert st0 == st1 == st2 == 200 and st3 == 400 and b"`level`" in msg
    assert plain == off and "x-smtts-start" not in h0 and "x-smtts-start" not in h1 and "x-smtts-samples" not in h1
    s, n = int(h2["x-smtts-start"]), int(h2["x-smtts-samples"])
    full = np.frombuffer(plain[44:], "<i2")
    assert full.size == 3200 * S.frames_for(1.3) and full.any() and 0 <= s and s + n <= full.size
    assert np.array_equal(np.frombuffer(cut[44:], "<i2"), full[s:s + n]) and len(cut) == 44 + 2 * n
    y, (yt, st), (yl, sl) = futs
    assert np.array_equal(np.trunc(np.clip(y, -1, 1) * 32767.0).astype("<i2"), full)
    seg, gain, _, _ = run_endpoints(eng, [(y, y.size)], Endpointing(level_dbfs=-20, **SHARP))
    assert (st, yt.size) == (sl, yl.size) == (int(seg[0, 0]), int(seg[0, 1]))
    assert np.array_equal(yt, y[st:st + yt.size]) and np.array_equal(yl, y[sl:sl + yl.size] * np.float32(gain[0]))
    print(f"server: default trim kept {n} of {full.size} samples from {s}; sharp trim kept {yt.size} from {st}, gain {gain[0]:.3f}")
