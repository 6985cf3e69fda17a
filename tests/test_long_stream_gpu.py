"""GPU: streamed long-form synthesis (include/smalltts_hip.h smtts_join_stream).  The running join against its numpy
restatement (tests/helpers/join_stream_ref.py) bit for bit (single fp32 multiplies: no tolerance), its carried state against
smtts_stitch_seg writing the same windows at plan_packed's offsets into one buffer, delivery from the device table against one
delivery of the whole joined buffer, guard bands, truncation and refusals; then the generator on the small engine of
tests/test_longform_gpu.py against synthesize_long, and the CLI."""
import ctypes as C

import numpy as np
import pytest
import torch

from smalltts_amd import audio as A
from smalltts_amd.api import Delivery, Endpointing, plan_packed, stream_groups
from smalltts_amd.weights import CodecSpec
from tests.helpers import join_stream_ref as J
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
ROW = 700


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def snr_db(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return 10 * np.log10((ref ** 2).sum() / max(((got - ref) ** 2).sum(), 1e-300))


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


def _fade(F):
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(F, dtype=np.float64) + 0.5) / max(F, 1))).astype(np.float32)[:F]


def _call(seed, seg, nan_outside=False):
    """-> (audio (B,1,ROW) with samples of +-4 among the noise (the PCM16 clamp), seg, gain)"""
    g = np.random.default_rng(seed)
    B = len(seg)
    audio = g.uniform(-1.0, 1.0, (B, 1, ROW)).astype(np.float32)
    audio[:, 0, ::13] = 4.0
    audio[:, 0, 5::17] = -4.0
    if nan_outside:
        keep = np.zeros((B, 1, ROW), bool)
        for b, (s, n) in enumerate(seg):
            keep[b, 0, s:s + n] = True
        audio[~keep] = np.nan
    return audio, [tuple(w) for w in seg], g.uniform(0.5, 1.5, B).astype(np.float32)


# windows of one row of 700: n = 0, n = 1, n < 2F (F = 16), start + n = row_stride, and 255 / 256 / 257 around a tile edge of 256
CALL_A = [(3, 0), (10, 1), (100, 20), (40, 255), (5, 256)]
CALL_B = [(ROW - 257, 257), (0, 0), (ROW - 1, 1), (444, 256), (0, ROW)]


def _join(eng, state, call, gap, F, with_gain, pcm16, **kw):
    audio, seg, gain = call
    fade = torch.from_numpy(_fade(F)).to(eng.device) if F else None
    return eng.join_stream(torch.from_numpy(audio).to(eng.device), torch.tensor(seg, dtype=torch.int64, device=eng.device),
                           torch.from_numpy(gain).to(eng.device) if with_gain else None, fade, gap, state, pcm16=pcm16, **kw)


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("gap", [0, 37])
@pytest.mark.parametrize("F", [0, 16])
@pytest.mark.parametrize("with_gain", [False, True])
def test_kernel_equals_the_restatement_bit_for_bit(eng, pcm16, gap, F, with_gain):
    state, ref = eng.join_state(), (0, 0)
    for c, seg in enumerate((CALL_A, CALL_B)):
        call = _call(10 + c, seg)
        chunk, off, rec, dtable = _join(eng, state, call, gap, F, with_gain, pcm16, last=bool(c), deliver_slot=3)
        ref, want, w_off, w_rec, w_dt = J.join_call(ref, call[0], seg, call[2] if with_gain else None, _fade(F), gap, pcm16, last=bool(c), slot=3)
        assert tuple(rec.tolist()) == w_rec and off.tolist() == w_off and tuple(dtable.tolist()) == w_dt and tuple(state.tolist()) == ref
        got = chunk[: w_rec[1] - w_rec[0]].cpu().numpy()
        assert got.dtype == want.dtype and chunk.numel() == 5 * (ROW + gap)
        assert np.array_equal(got.view(np.uint32 if not pcm16 else np.int16), want.view(np.uint32 if not pcm16 else np.int16)), (c, int((got != want).sum()))


# ---- carried state --------------------------------------------------------------------------------------------------------------------
def _three_calls(variant):
    segs = [[(7, 300), (0, 0), (450, 250)], [(100, 257)], [(0, 1), (600, 100), (3, 0), (0, ROW)]]
    if variant == "empty_first":
        segs[0] = [(7, 0), (0, 0), (450, 0)]
    if variant == "empty_middle":
        segs[1] = [(100, 0)]
    return [_call(20 + c, s) for c, s in enumerate(segs)]


@pytest.mark.parametrize("variant", ["plain", "empty_first", "empty_middle"])
@pytest.mark.parametrize("pcm16", [False, True])
def test_carried_state_equals_stitch_seg_at_plan_packed_offsets(eng, variant, pcm16):
    calls, gap, F = _three_calls(variant), 37, 16
    all_n = [n for _a, seg, _g in calls for _s, n in seg]
    offsets, S = plan_packed(all_n, gap * 1000.0 / 24000.0)
    fade = torch.from_numpy(_fade(F)).to(eng.device)
    whole = torch.zeros(S, dtype=torch.int16 if pcm16 else torch.float32, device=eng.device)
    state, ref, chunks, at = eng.join_state(), (0, 0), [], 0
    for c, call in enumerate(calls):
        audio, seg, gain = call
        eng.stitch_seg(torch.from_numpy(audio).to(eng.device), torch.tensor(seg, dtype=torch.int64, device=eng.device),
                       torch.from_numpy(gain).to(eng.device), offsets[at: at + len(seg)], fade, whole)
        chunk, off, rec, _dt = _join(eng, state, call, gap, F, True, pcm16, last=c == 2)
        ref, _w, w_off, w_rec, _d = J.join_call(ref, audio, seg, gain, _fade(F), gap, pcm16)
        assert off.tolist() == offsets[at: at + len(seg)] == w_off and tuple(rec.tolist()) == w_rec and tuple(state.tolist()) == ref
        chunks.append(chunk[: w_rec[1] - w_rec[0]])
        at += len(seg)
    assert ref == (S, sum(n > 0 for n in all_n))
    got, want = torch.cat(chunks).cpu().numpy(), whole.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got.view(np.int16 if pcm16 else np.uint32), want.view(np.int16 if pcm16 else np.uint32))


def test_snapshot_reproduces_a_chunk_and_states_do_not_see_each_other(eng):
    calls, gap, F = _three_calls("plain"), 37, 16
    state = eng.join_state()
    _join(eng, state, calls[0], gap, F, True, False, last=False)
    snap = state.clone()
    a, a_off, a_rec, _ = _join(eng, state, calls[1], gap, F, True, False, last=False)
    b, b_off, b_rec, _ = _join(eng, snap.clone(), calls[1], gap, F, True, False, last=False)
    assert torch.equal(a_rec, b_rec) and torch.equal(a_off, b_off) and torch.equal(a[: 257 + gap].view(torch.int32), b[: 257 + gap].view(torch.int32))
    z, z_off, z_rec, _ = _join(eng, eng.join_state(), calls[1], gap, F, True, False, last=False)
    assert z_rec.tolist() == [0, 257, 0, 1] and a_rec.tolist() == [550 + gap, 550 + 257 + 2 * gap, 2, 3]     # a zeroed slot: no gap in front
    assert not torch.equal(a[:257].view(torch.int32), z[:257].view(torch.int32)) and float(a[:gap].abs().max()) == 0.0
    # two states advanced in alternation: each is the restatement of its own sequence
    sa, sb, ra, rb = eng.join_state(), eng.join_state(), (0, 0), (0, 0)
    for c in range(3):
        ca, cb = calls[c], calls[2 - c]
        ga, _o, rec_a, _ = _join(eng, sa, ca, gap, F, False, False, last=False)
        gb, _o, rec_b, _ = _join(eng, sb, cb, 5, 0, True, True, last=False)
        ra, wa, _o, w_rec_a, _ = J.join_call(ra, ca[0], ca[1], None, _fade(F), gap)
        rb, wb, _o, w_rec_b, _ = J.join_call(rb, cb[0], cb[1], cb[2], None, 5, True)
        assert tuple(rec_a.tolist()) == w_rec_a and tuple(rec_b.tolist()) == w_rec_b
        assert np.array_equal(ga[: len(wa)].cpu().numpy().view(np.uint32), wa.view(np.uint32)) and np.array_equal(gb[: len(wb)].cpu().numpy(), wb)
    assert tuple(sa.tolist()) == ra and tuple(sb.tolist()) == rb


# ---- delivery from the device table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate, encoding", [(8000, "mulaw"), (48000, "pcm16"), (24000, "pcm16")])
def test_join_then_deliver_from_the_table_equals_one_delivery_of_the_whole(eng, rate, encoding):
    calls, gap, F, zeros = _three_calls("plain"), 37, 16, 3
    up, down = A.deliver_ratio(rate)
    width = 0 if (up, down) == (1, 1) else A._sinc_kernel(down, up, zeros)[1]
    empty = (calls[0][0], [(0, 0)] * 3, calls[0][2])                     # a final all-empty call with `last`: the pure flush
    state = eng.join_state()
    dstate = eng.deliver_state(1, rate, zeros)
    assert (dstate is None) == (rate == 24000)
    joined, outs = [], []
    for c, call in enumerate(calls + [empty]):
        last = c == 3
        chunk, _off, rec, dtable = _join(eng, state, call, gap, F, True, False, last=last, deliver_slot=0)
        out = eng.deliver_from_table(chunk, dtable, rate, encoding, state=dstate, zeros=zeros)
        p0, p1 = rec[:2].tolist()
        assert dtable.tolist() == [0, p0, p1 - p0, int(last)]
        cnt = p1 - p0 if rate == 24000 else A.deliver_counts(p0, p1 - p0, last, up, down, width)
        assert tuple(out.shape) == (1, max(1, A.deliver_max_count(chunk.numel(), up, down, width, dstate is not None)))
        joined.append(chunk[: p1 - p0])
        outs.append(out[0, :cnt])
    whole = torch.cat(joined)
    S = whole.numel()
    want, cnt = eng.deliver(whole.view(1, 1, S), [S], rate, encoding, zeros=zeros)
    got = torch.cat(outs).cpu().numpy()
    assert got.shape[0] == cnt[0] and got.tobytes() == want[0, : cnt[0]].cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        eng.deliver_from_table(whole, dtable[:3], rate, encoding, zeros=zeros)
    if rate == 24000:
        with pytest.raises(ValueError):
            eng.deliver_from_table(whole, dtable, rate, encoding, state=eng.deliver_state(1, 8000, zeros), zeros=zeros)


# ---- guard bands, truncation, refusals ----------------------------------------------------------------------------------------------
class _Raw:
    """One smtts_join_stream call on guarded buffers."""

    def __init__(self, eng, call, gap, F, pcm16, cap, with_gain=True, with_dtable=True):
        self.eng, self.gap, self.F, self.pcm16, self.cap = eng, gap, F, pcm16, cap
        audio, seg, gain = call
        self.B = len(seg)
        a = self.a = Arena(eng.device)
        self.audio = a.put("audio", torch.from_numpy(audio))
        self.seg = a.put("seg", torch.tensor(seg, dtype=torch.int64))
        self.gain = a.put("gain", torch.from_numpy(gain)) if with_gain else None
        self.fade = a.put("fade", torch.from_numpy(_fade(F))) if F else None
        self.state = a.alloc("state", (2,), torch.int64, role="in")
        self.chunk = a.alloc("chunk", (cap,), torch.int16 if pcm16 else torch.float32)
        self.off = a.alloc("off", (self.B,), torch.int64)
        self.rec = a.alloc("rec", (4,), torch.int64)
        self.dtable = a.alloc("dtable", (4,), torch.int64) if with_dtable else None

    def args(self, **over):
        d = dict(audio=self.audio, B=self.B, row_stride=ROW, seg=self.seg, gain=self.gain, fade=self.fade, F=self.F, gap=self.gap, last=1,
                 state=self.state, chunk=self.chunk, cap=self.cap, pcm16=int(self.pcm16), off=self.off, rec=self.rec, dtable=self.dtable, slot=9)
        d.update(over)
        return d

    def run(self, **over):
        d, e = self.args(**over), self.eng
        ptr = lambda v: v if isinstance(v, C.c_void_p) else _p(v)
        return e.lib.smtts_join_stream(e.h, e._stream(), ptr(d["audio"]), d["B"], d["row_stride"], ptr(d["seg"]), ptr(d["gain"]), ptr(d["fade"]),
                                       d["F"], d["gap"], d["last"], ptr(d["state"]), ptr(d["chunk"]), d["cap"], d["pcm16"], ptr(d["off"]),
                                       ptr(d["rec"]), ptr(d["dtable"]), d["slot"])


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("with_gain", [False, True])
def test_guard_bands_nothing_outside_and_nan_behind_every_window(eng, pcm16, with_gain):
    gap, F = 37, 16
    call = _call(31, CALL_A[1:] + [(ROW - 257, 257)], nan_outside=True)
    _s, want, w_off, w_rec, w_dt = J.join_call((1000, 2), call[0], call[1], call[2] if with_gain else None, _fade(F), gap, pcm16, last=True, slot=9)
    n = want.shape[0]
    k = _Raw(eng, call, gap, F, pcm16, cap=n + 300, with_gain=with_gain)
    k.a.claim("chunk", n * want.dtype.itemsize)                     # what lies behind the chunk's length counts as guard
    snaps = []
    for byte in (0x00, 0xFF):
        k.a.paint(byte)
        k.state.copy_(torch.tensor([1000, 2]))
        assert k.run() == 0, eng.lib.smtts_last_error(eng.h)
        torch.cuda.synchronize()
        k.a.assert_clean("smtts_join_stream", f"pcm16 {pcm16} gain {with_gain} (guards 0x{byte:02X})")
        snaps.append([t.cpu().numpy().copy() for t in (k.chunk[:n], k.off, k.rec, k.dtable, k.state)])
    for x, y in zip(*snaps):
        assert x.tobytes() == y.tobytes()
    got, off, rec, dtable, state = snaps[0]
    assert got.tobytes() == want.tobytes() and not np.isnan(got.astype(np.float64)).any()
    assert off.tolist() == w_off and tuple(rec.tolist()) == w_rec and tuple(dtable.tolist()) == w_dt and state.tolist() == [w_rec[1], w_rec[3]]


@pytest.mark.parametrize("pcm16", [False, True])
def test_truncation_drops_the_last_sample_and_rec_is_untruncated(eng, pcm16):
    gap, F = 37, 0
    call = _call(32, CALL_B)
    _s, want, w_off, w_rec, _d = J.join_call((0, 0), call[0], call[1], None, None, gap, pcm16)
    n = want.shape[0]
    k = _Raw(eng, call, gap, F, pcm16, cap=n - 1, with_gain=False, with_dtable=False)
    k.a.paint(0xFF)
    k.state.zero_()
    assert k.run() == 0, eng.lib.smtts_last_error(eng.h)
    torch.cuda.synchronize()
    k.a.assert_clean("smtts_join_stream", f"cap one short, pcm16 {pcm16}")
    assert k.chunk.cpu().numpy().tobytes() == want[: n - 1].tobytes()
    assert tuple(k.rec.tolist()) == w_rec == (0, n, 0, 4) and k.off.tolist() == w_off and k.state.tolist() == [n, 4]


def test_refusals_return_1_name_the_entry_and_enqueue_nothing(eng):
    lib = eng.lib
    k = _Raw(eng, _call(33, CALL_A), 37, 16, False, cap=5 * (ROW + 37))
    k.a.paint(0xFF)
    k.state.copy_(torch.tensor([12, 1]))
    odd = torch.zeros(3, dtype=torch.int64, device=eng.device)
    odd_state = odd[1:] if odd.data_ptr() % 16 == 0 else odd[:2]
    assert odd_state.data_ptr() % 16 == 8
    bad = [dict(audio=None), dict(seg=None), dict(off=None), dict(rec=None), dict(chunk=None), dict(state=None), dict(state=odd_state),
           dict(B=0), dict(B=1025), dict(B=-1), dict(row_stride=0), dict(row_stride=(1 << 40) + 1), dict(gap=-1), dict(gap=(1 << 31) + 1),
           dict(F=-1), dict(fade=None), dict(cap=0), dict(cap=-5)]
    for over in bad:
        assert k.run(**over) == 1, over
        assert b"smtts_join_stream" in lib.smtts_last_error(eng.h), (over, lib.smtts_last_error(eng.h))
    assert lib.smtts_join_stream(None, *([None] * 2), 5, ROW, *([None] * 3), 0, 0, 0, None, None, 1, 0, None, None, None, 0) == 1
    assert b"smtts_join_stream" in lib.smtts_last_error(None)
    torch.cuda.synchronize()
    k.a.assert_clean("smtts_join_stream", "refusals")
    assert k.state.tolist() == [12, 1] and not k.chunk.any() and not k.off.any() and not k.rec.any() and not k.dtable.any()   # as painted
    assert not odd.any()
    assert k.run() == 0 and k.run(dtable=None, gain=None, F=0, fade=None, gap=0) == 0            # the limits' good side
    torch.cuda.synchronize()
    k.a.assert_clean("smtts_join_stream", "good")
    with pytest.raises(ValueError):
        eng.join_stream(k.audio, k.seg, None, None, 0, odd_state, last=False, pcm16=False)
    with pytest.raises(ValueError):
        eng.join_stream(k.audio, k.seg[:4], None, None, 0, eng.join_state(), last=False, pcm16=False)
    with pytest.raises(ValueError):
        eng.join_stream(k.audio, k.seg, None, None, -1, eng.join_state(), last=False, pcm16=False)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
G = np.random.default_rng(12)
DURS = [0.3, 0.55, 0.45, 0.3, 0.4]                                       # 2, 4, 3, 2, 3 frames
TOKS = [[int(t) for t in G.integers(1, 198, size=int(G.integers(3, 12)))] for _ in DURS]
LONG_KW = dict(token_lists=TOKS, durations=DURS, seed=3, max_batch=2, in_flight=2, gap_ms=20.0, fade_ms=2.0)
CASES = {
    "plain": {},
    "pcm16": dict(pcm16=True),
    "trim": dict(trim=True),
    "trim_level": dict(trim=Endpointing(level_dbfs=-23.0)),
    "words": dict(return_words=True),
    "mulaw_8k": dict(deliver=Delivery(8000, "mulaw")),
    "pcm16_48k": dict(deliver=(48000, "pcm16")),
}


def _same_pieces(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.tokens == y.tokens and x.prefix_len == y.prefix_len and x.seed == y.seed and np.array_equal(x.latents, y.latents)
        assert (x.spans is None) == (y.spans is None) and (x.spans is None or np.array_equal(x.spans, y.spans))


@pytest.mark.parametrize("case", list(CASES))
def test_chunks_are_synthesize_long_bit_for_bit(eng, tts, voice, case):
    kw = dict(LONG_KW, **CASES[case])
    words = kw.get("return_words", False)
    res = tts.synthesize_long(voice, return_segments=True, return_pieces=True, **kw)
    want, segs, pieces = res[0], res[1], res[-1]
    chunks = list(tts.synthesize_long_stream(voice, return_pieces=True, batch_sizes=None, **kw))
    assert [c.index for c in chunks] == [0, 1, 2] and [len(c.segments) for c in chunks] == [2, 2, 1]
    got = np.concatenate([c.audio for c in chunks], 1)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), case
    assert want.shape[1] > 0 and want.any()
    assert [s for c in chunks for s in c.segments] == segs
    if words:
        assert [w for c in chunks for w in c.words] == res[2] and len(res[2]) > 0
    else:
        assert all(c.words is None for c in chunks)
    _same_pieces([p for c in chunks for p in c.pieces], pieces)
    pos = 0
    for c in chunks:                                                    # offsets count what was handed out before the chunk
        assert c.offset == pos and c.audio.shape[0] == 1
        pos += c.audio.shape[1]
    assert getattr(eng, "tuning", "latency") == "latency" and eng._ws_slot is None


def test_default_ramp_groups_offsets_segments_and_regrouping_tolerance(eng, tts, voice):
    """Another grouping changes batch shapes: the bar is test_longform_gpu.py's `max_batch = 1 vs 8` one, 80 dB."""
    kw = dict(LONG_KW, max_batch=8)
    want = tts.synthesize_long(voice, **kw)
    chunks = list(tts.synthesize_long_stream(voice, **kw))
    groups = stream_groups(5, (1, 2, 4, 8), 8)
    assert [len(g) for g in groups] == [1, 2, 2] and [len(c.segments) for c in chunks] == [len(g) for g in groups]
    assert all(c.words is None and c.pieces is None for c in chunks)
    gap, pos, at = round(20.0 * 24), 0, 0
    frames = [2, 4, 3, 2, 3]
    for c in chunks:                                                    # offsets are contiguous ...
        assert c.offset == pos
        pos += c.audio.shape[1]
        for off, n, start, gain in c.segments:                          # ... and the segments tile the stream, `gap` between the pieces
            assert (off, n, start, gain) == (sum(3200 * f + gap for f in frames[:at]), 3200 * frames[at], 0, 1.0)
            at += 1
        assert pos == off + n                                           # a chunk ends where its last piece ends
    got = np.concatenate([c.audio for c in chunks], 1)
    assert got.shape == want.shape
    s = snr_db(got, want)
    print(f"\n[long stream] default ramp vs synthesize_long: {s:.1f} dB")
    assert s > 80.0, s
    assert list(tts.synthesize_long_stream(voice, token_lists=[], durations=[])) == []      # empty text yields nothing
    with pytest.raises(ValueError):
        tts.synthesize_long_stream(voice, pcm16=True, deliver=8000, **LONG_KW)               # refused before the first next()


def test_closing_after_the_first_chunk_leaves_the_engine_as_a_finished_call_does(eng, tts, voice):
    kw = dict(LONG_KW, trim=True)
    before = tts.synthesize_long(voice, **kw)
    prev = eng.set_tuning("throughput")                                  # a caller's own tuning must come back, whichever it is
    try:
        gen = tts.synthesize_long_stream(voice, batch_sizes=None, **kw)
        first = next(gen)
        gen.close()
        assert eng.tuning == "throughput" and eng._ws_slot is None
    finally:
        eng.set_tuning(prev)
    assert first.index == 0 and first.audio.tobytes() == before[:, : first.audio.shape[1]].tobytes()
    assert tts.synthesize_long(voice, **kw).tobytes() == before.tobytes()


def test_a_demotion_while_groups_are_in_flight_runs_them_again_and_the_stream_is_the_demoted_engines():
    """The fp16 range guard inside the generator, on weights known to clamp (tests/test_api_rerun_gpu.py's engine and its A / B scheme):
    call A's first verification demotes the site with two groups in flight, they run again in order on the caller's stream and the
    third group runs at the demoted precision; call B runs once on the demoted engine.  Every element of every chunk is equal, and the
    chunks are the demoted engine's synthesize_long."""
    from tests.test_api_rerun_gpu import FRAMES, TOKS, TRIM, _twice
    ns = [FRAMES[0], FRAMES[1], FRAMES[0], FRAMES[1], FRAMES[0]]
    toks = [TOKS[i % 4] for i in range(5)]

    def call(tts, voice):
        kw = dict(token_lists=toks, durations=[(n + 0.5) / 7.5 for n in ns], seed=5, max_batch=2, in_flight=2, trim=TRIM, return_words=True)
        chunks = list(tts.synthesize_long_stream(voice, batch_sizes=None, return_pieces=True, **kw))
        wave, segs, words = tts.synthesize_long(voice, return_segments=True, **kw)     # (the engine is demoted by now in A too)
        assert np.concatenate([c.audio for c in chunks], 1).tobytes() == wave.tobytes()
        assert [s for c in chunks for s in c.segments] == segs and [w for c in chunks for w in c.words] == words
        return chunks
    chunks = _twice(call, tuning="throughput")
    assert [len(c.segments) for c in chunks] == [2, 2, 1] and [len(c.pieces) for c in chunks] == [2, 2, 1]


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delivery", [[], ["--rate", "8000", "--encoding", "mulaw"]])
def test_longform_cli_stream_writes_the_same_file(tmp_path, delivery, capsys):
    from smalltts_amd.audio import write_wav_pcm16
    from smalltts_amd.scripts import longform as L
    sr = 16000
    t = np.arange(int(0.9 * sr)) / sr
    write_wav_pcm16(str(tmp_path / "ref.wav"), 0.5 * np.sin(2 * np.pi * 440 * t), sr)
    (tmp_path / "tokens.txt").write_text("1,2,3,4,5,6,7,8\n10,20,30,40\n\n5,9,14,33,41,14,77,120,3\n")
    base = ["--wav", str(tmp_path / "ref.wav"), "--tokens-file", str(tmp_path / "tokens.txt"), "--durations", "0.4,0.3,0.5", "--weights",
            "synthetic:3", "--precision", "bf16x3", "--seed", "0", "--gap-ms", "100", "--max-batch", "2", "--in-flight", "2", "--trim"] + delivery
    L.main(base + ["--out", str(tmp_path / "whole.wav")])
    L.main(base + ["--out", str(tmp_path / "stream.wav"), "--stream", "--batch-sizes", "none"])
    said = capsys.readouterr().out
    assert "first chunk after" in said
    a, b = (tmp_path / "whole.wav").read_bytes(), (tmp_path / "stream.wav").read_bytes()
    assert len(a) > 44 + 1000 and a == b
