"""GPU: long-form synthesis: a voice encoded once (voice_expand), per-row noise (randn_rows), rows joined on the device (stitch), and
the Python surface on top (Voice, synthesize_batch(voices=, seeds=), synthesize_long, the longform CLI).  The engine is built like
tests/test_api_gpu.py's (split-bf16, seed 11, the tiny codec): the two bars quoted below were set on that configuration."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dit_oracle as O
from smalltts_amd.weights import CodecSpec, dit_param_specs, synth_state_dict
from tests.conftest import rel_l2
from tests.helpers.longform_ref import STITCH_CASES, pcm16_numpy, stitch_case, stitch_numpy

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11


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
def refs():
    g = np.random.default_rng(0)
    return [g.standard_normal((r, 64)).astype(np.float32) for r in (5, 9, 7)]


@pytest.fixture(scope="module")
def voices(tts, refs):
    return [tts.encode_voice(r) for r in refs]


def test_voice_expand_is_a_copy(eng, voices, refs):
    rows = [0, 1, 0, 2]
    out = eng.voice_expand([voices[i] for i in rows])
    torch.cuda.synchronize()
    assert [v.R for v in voices] == [5, 9, 7] and tuple(voices[1].k_ref.shape) == (12, 1, 8, 9, 120)
    assert tuple(out["k_ref"].shape) == tuple(out["v_ref"].shape) == (12, 4, 8, 9, 120) and tuple(out["ref_mask"].shape) == (4, 9)
    for b, i in enumerate(rows):
        R = voices[i].R
        for name in ("k_ref", "v_ref"):
            assert torch.equal(out[name][:, b, :, :R], getattr(voices[i], name)[:, 0]), (name, b)
            assert float(out[name][:, b, :, R:].abs().max()) == 0.0 if R < 9 else True
        assert out["ref_mask"][b].tolist() == [j < R for j in range(9)]
    # the mask cond_encode returns for the same lengths
    lens = [voices[i].R for i in rows]
    ref = np.zeros((4, 9, 64), np.float32)
    for b, i in enumerate(rows):
        ref[b, :lens[b]] = refs[i]
    want = eng.cond_encode(ref, np.asarray(lens), np.zeros((4, 0), np.int64), np.zeros((4, 0), bool))["ref_mask"]
    assert torch.equal(out["ref_mask"], want)
    with pytest.raises(AttributeError):
        voices[0].R = 3
    # one row, and a voice that is a view at an odd (4-byte) address: the scalar path copies the same values
    odd = torch.zeros(voices[2].k_ref.numel() + 1, device=eng.device)
    odd[1:] = voices[2].k_ref.reshape(-1)
    one = eng.voice_expand([(odd[1:].view(12, 1, 8, 7, 120), voices[2].v_ref)])
    assert torch.equal(one["k_ref"], voices[2].k_ref) and torch.equal(one["v_ref"], voices[2].v_ref) and bool(one["ref_mask"].all())


def test_voice_alone_equals_the_reference_half_of_a_padded_batch(eng, voices, refs):
    """Same math, another batch shape: the bar of tests/test_dit_gpu.py::test_ragged_batch_equals_per_utterance (2e-5)."""
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(1, 198, (3, 6), generator=g)
    pm = torch.ones(3, 6, dtype=torch.bool)
    ref = np.zeros((3, 9, 64), np.float32)
    for b, r in enumerate(refs):
        ref[b, :r.shape[0]] = r
    full = eng.cond_encode(ref, np.asarray([5, 9, 7]), ids, pm)
    out = eng.voice_expand(voices)
    assert torch.equal(out["ref_mask"], full["ref_mask"])
    for b, R in enumerate((5, 9, 7)):
        for name in ("k_ref", "v_ref"):
            err = rel_l2(out[name][:, b, :, :R].cpu().numpy(), full[name][:, b, :, :R].cpu().numpy())
            print(f"voice {b} {name}: alone vs padded batch rel L2 = {err:.3e}")
            assert err < 2e-5, (b, name, err)


@pytest.mark.parametrize("tuning", ["latency", "throughput"])
def test_text_half_alone_is_bit_identical(eng, refs, tuning):
    g = torch.Generator().manual_seed(6)
    ids = torch.randint(1, 198, (3, 10), generator=g)
    pm = torch.zeros(3, 10, dtype=torch.bool)
    for b, p in enumerate((4, 10, 7)):
        pm[b, :p] = True
    ids = ids * pm
    ref = np.zeros((3, 9, 64), np.float32)
    for b, r in enumerate(refs):
        ref[b, :r.shape[0]] = r
    prev = eng.set_tuning(tuning)
    try:
        full = eng.cond_encode(ref, np.asarray([5, 9, 7]), ids, pm)
        text = eng.cond_encode(np.zeros((3, 0, 64), np.float32), np.zeros(3, np.int64), ids, pm)
        torch.cuda.synchronize()
    finally:
        eng.set_tuning(prev)
    assert tuple(text["k_ref"].shape) == (12, 3, 8, 0, 120)
    assert torch.equal(text["k_text"], full["k_text"]) and torch.equal(text["v_text"], full["v_text"])


def test_randn_rows_equals_the_per_row_loop(eng):
    from oracle.philox import philox_randn
    ns, steps, seeds = (7, 16, 11), 4, (1234, 2 ** 63 - 5, 99)
    got = eng.randn_rows(seeds, ns, steps)
    want = torch.zeros(steps, 3, 16, 64, device=eng.device)
    for b in range(3):
        for s in range(steps):
            want[s, b, :ns[b]] = eng.randn(ns[b] * 64, seeds[b], s).view(ns[b], 64)
    assert tuple(got.shape) == (4, 3, 16, 64) and torch.equal(got, want)
    assert float(got[:, 0, 7:].abs().max()) == 0.0 and float(got[:, 2, 11:].abs().max()) == 0.0
    for s in range(steps):
        ref = philox_randn(16 * 64, seeds[1], s)
        assert np.abs(got[s, 1].reshape(-1).cpu().numpy() - ref).max() < 2e-5
    # a wider padding than the longest row, and a different order: every row is the same
    wide = eng.randn_rows(seeds[::-1], ns[::-1], steps, n_max=20)
    assert torch.equal(wide[:, 2, :7], got[:, 0, :7]) and torch.equal(wide[:, 0, :11], got[:, 2, :11]) and float(wide[:, :, 16:].abs().max()) == 0.0


@pytest.mark.parametrize("case", range(len(STITCH_CASES)))
@pytest.mark.parametrize("pcm16", [False, True])
def test_stitch_bit_for_bit(eng, case, pcm16):
    hop, batches, F, gap = STITCH_CASES[case]
    rows, fade, S = stitch_case(hop, batches, F, gap, seed=case)
    dt = np.int16 if pcm16 else np.float32
    want = np.zeros(S, dt)
    out = torch.zeros(S, dtype=torch.int16 if pcm16 else torch.float32, device=eng.device)
    fade_d = torch.from_numpy(fade).to(eng.device) if F else None
    real_hop = eng.hop
    for audio, lens, offs in rows:          # several batches write into the one buffer
        stitch_numpy(want, audio, lens, offs, fade)
        ns = [n // hop for n in lens]
        if hop == real_hop:
            eng.stitch(torch.from_numpy(audio).to(eng.device), ns, offs, fade_d, out)
        else:                               # other hops than the codec's: through the C entry, which takes samples
            import ctypes as C
            a = torch.from_numpy(audio).to(eng.device)
            tab = torch.tensor([lens, offs], dtype=torch.int64, device=eng.device)
            p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
            rc = eng.lib.smtts_stitch(eng.h, eng._stream(), p(a), a.shape[0], a.shape[-1], p(tab[0]), p(tab[1]), p(fade_d), F, p(out),
                                      S, int(pcm16))
            assert rc == 0, eng.lib.smtts_last_error(eng.h)
    got = out.cpu().numpy()
    assert np.array_equal(got, want), (case, pcm16, int((got != want).sum()))


def test_voices_equal_ref_latents_and_the_oracle(eng, tts, voices, refs):
    """The voice path against the reference-latents path on the same explicit noise: the padded-batch-vs-single bar of
    test_reference_api_shapes_and_batch_equals_single (80 dB), and the end-to-end oracle bar of
    test_synthesize_matches_oracle_end_to_end (latents 1e-4)."""
    g = np.random.default_rng(0)
    toks = [[1, 2, 3, 4], [10, 20, 30, 40, 50, 60], [7] * 9]
    durs = [1.0, 2.2, 1.5]
    ns = [7, 16, 11]
    noise = g.standard_normal((4, 3, 16, 64)).astype(np.float32)
    want, want_lat = tts.synthesize_batch(refs, toks, durs, noise=noise, return_latents=True)
    got, got_lat = tts.synthesize_batch(None, toks, durs, noise=noise, voices=voices, return_latents=True)
    assert [o.shape for o in got] == [(1, 3200 * n) for n in ns]
    for b in range(3):
        s = snr_db(got[b], want[b])
        print(f"row {b}: voices= vs ref_latents= {s:.1f} dB, latents rel L2 {rel_l2(got_lat[b], want_lat[b]):.3e}")
        assert s > 80.0, (b, s)
    w = O.to_torch(synth_state_dict(dit_param_specs(), SEED))
    for b in range(3):          # the oracle on each utterance alone, unpadded, as the end-to-end test of the reference-latents path does
        with torch.no_grad():
            pm = torch.ones(1, len(toks[b]), dtype=torch.bool)
            cache = O.encode_conditions(w, torch.from_numpy(refs[b])[None], torch.tensor([refs[b].shape[0]]), torch.tensor([toks[b]]), pm)
            x = O.sample_dmd(w, cache, pm, torch.ones(1, ns[b], dtype=torch.bool), torch.from_numpy(noise[:, b:b + 1, :ns[b]].copy()), 4)
        err = rel_l2(got_lat[b], x[0].numpy())
        print(f"row {b}: voices= latents vs oracle rel L2 = {err:.3e}")
        assert err < 1e-4, (b, err)
    with pytest.raises(ValueError):
        tts.synthesize_batch(refs, toks, durs, voices=voices)
    with pytest.raises(ValueError):
        tts.synthesize_batch(refs, toks, durs, noise=noise, seeds=[1, 2, 3])


def test_seeds_make_a_row_independent_of_its_batch_mates(eng, tts, voices):
    toks = [[1, 2, 3, 4], [10, 20, 30, 40, 50, 60], [7] * 9]
    durs = [1.0, 2.2, 1.5]
    _, a = tts.synthesize_batch(None, toks, durs, voices=voices, seeds=[5, 6, 7], return_latents=True)
    _, b = tts.synthesize_batch(None, toks, durs, voices=voices, seeds=[5, 600, 700], return_latents=True)
    _, c = tts.synthesize_batch(None, toks, durs, voices=voices, seeds=[5, 6, 7], return_latents=True)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    for r in range(3):
        _, one = tts.synthesize_batch(None, [toks[r]], [durs[r]], voices=[voices[r]], seeds=[[5, 6, 7][r]], return_latents=True)
        err = rel_l2(a[r], one[0])
        print(f"row {r}: in the batch vs alone, same seed: rel L2 = {err:.3e}")
        assert err < 2e-5, (r, err)


def test_synthesize_long_equals_the_hand_made_composition(eng, tts, voices):
    from smalltts_amd.api import HOP_SIZE, fade_table, piece_seed, plan_long
    g = np.random.default_rng(12)
    durs = [1.0, 2.2, 1.5, 0.7, 3.0, 1.2, 2.0, 0.5, 1.8, 2.6, 0.9]
    ns = [max(1, int(d * 7.5)) for d in durs]
    toks = [[int(t) for t in g.integers(1, 198, size=int(g.integers(3, 20)))] for _ in durs]
    voice = voices[1]
    kw = dict(token_lists=toks, durations=durs, seed=3)
    out = tts.synthesize_long(voice, **kw)
    gap = round(120.0 * 24)
    S = sum(HOP_SIZE * n for n in ns) + 10 * gap
    assert out.shape == (1, S) and out.dtype == np.float32 and np.isfinite(out).all()
    assert eng.tuning == "latency" if hasattr(eng, "tuning") else True      # the caller's tuning is restored
    # hand-made: every piece alone with its derived seed under the tuning synthesize_long runs its batches in, joined by numpy
    prev = eng.set_tuning("throughput")
    try:
        pieces = [tts.synthesize_batch(None, [toks[i]], [durs[i]], voices=[voice], seeds=[piece_seed(3, i)])[0] for i in range(11)]
    finally:
        eng.set_tuning(prev)
    _, offsets, S2 = plan_long(ns, 8, 120.0)
    assert S2 == S
    want = np.zeros(S, np.float32)
    for i, p in enumerate(pieces):
        stitch_numpy(want, p[None], [p.shape[1]], [offsets[i]], fade_table(5.0))
    s = snr_db(out[0], want)
    print(f"synthesize_long vs hand-made composition: {s:.1f} dB")
    assert s > 80.0, s
    for i in range(10):        # the gaps are silence
        lo = offsets[i] + HOP_SIZE * ns[i]
        assert not out[0, lo:lo + gap].any()
    one = tts.synthesize_long(voice, max_batch=1, **kw)
    s = snr_db(one[0], out[0])
    print(f"max_batch = 1 vs 8: {s:.1f} dB")
    assert s > 80.0, s
    assert np.array_equal(tts.synthesize_long(voice, **kw), out)
    pcm = tts.synthesize_long(voice, pcm16=True, **kw)
    assert pcm.dtype == np.int16 and pcm.shape == (1, S) and np.array_equal(pcm[0], pcm16_numpy(out[0]))
    assert np.array_equal(pcm[0], eng.pcm16(out[0]).cpu().numpy())
    # a prefix (the reference clip's transcription) is prepended to every piece
    pre = tts.synthesize_long(voice, token_lists=[t[2:] for t in toks], durations=durs, seed=3, prefix_tokens=[1, 2])
    same = tts.synthesize_long(voice, token_lists=[[1, 2] + t[2:] for t in toks], durations=durs, seed=3)
    assert np.array_equal(pre, same)
    with pytest.raises(ValueError):
        tts.synthesize_long(voice, "text", token_lists=toks, durations=durs)


def test_synthesize_long_from_text(eng, tts, voices, monkeypatch):
    """The text route: split_text -> tokens -> estimate_duration per piece (grapheme tokens here: no espeak offline)."""
    from smalltts_amd import phonemes
    from smalltts_amd.api import HOP_SIZE, estimate_duration, split_text
    chars = phonemes.get_token_ids
    monkeypatch.setattr(phonemes, "get_token_ids", lambda s, backend="chars": chars(s, backend="chars"))
    text = ("The engine speaks one utterance per row. A paragraph is cut at sentence ends, [laughter] then at commas, "
            "and only then at spaces! Short sentences share a row. " * 3)
    pieces = split_text(text)
    assert len(pieces) >= 3 and all(len(phonemes.get_token_ids(p)) <= 198 for p in pieces)
    out = tts.synthesize_long(voices[0], text, seed=1, gap_ms=50.0, fade_ms=0.0)
    ns = [max(1, int(estimate_duration(p) * 7.5)) for p in pieces]
    assert out.shape == (1, sum(HOP_SIZE * n for n in ns) + (len(ns) - 1) * 1200) and np.isfinite(out).all()
    # the prefix shrinks the splitter's budget by its length
    pre = tts.synthesize_long(voices[0], text, seed=1, prefix_tokens=list(range(1, 101)))
    assert pre.shape[1] > 0 and len(split_text(text, max_tokens=98)) > len(pieces)


def test_longform_cli_end_to_end(tmp_path):
    """longform.py surface: wav -> voice (resample, codec encode, style encoder once) -> pre-split token lists -> one PCM16 wav."""
    from smalltts_amd.audio import read_wav, write_wav_pcm16
    sr = 16000
    t = np.arange(int(0.9 * sr)) / sr
    write_wav_pcm16(str(tmp_path / "ref.wav"), 0.5 * np.sin(2 * np.pi * 440 * t), sr)
    with open(tmp_path / "tokens.txt", "w") as f:
        f.write("1,2,3,4,5,6,7,8\n10,20,30,40\n\n5,9,14,33,41,14,77,120,3\n")
    out = tmp_path / "out" / "long.wav"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "smalltts_amd.scripts.longform", "--wav", str(tmp_path / "ref.wav"), "--tokens-file",
                        str(tmp_path / "tokens.txt"), "--durations", "1.0,0.6,1.5", "--out", str(out), "--weights", "synthetic:3",
                        "--seed", "0", "--gap-ms", "100"], cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    a, rate = read_wav(str(out))
    assert rate == 24000 and a.shape == (3200 * (7 + 4 + 11) + 2 * 2400,) and np.isfinite(a).all()
    assert not a[3200 * 7:3200 * 7 + 2400].any() and a[:3200 * 7].any()
