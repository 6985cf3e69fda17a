"""GPU: alignment of long recordings through the Python API on synthetic weights with the recogniser part, the engines as
tests/test_align_api_gpu.py builds them.  engine.asr_logprobs_long is asr_logprobs per window plus numpy stitching by
plans.long_windows, bit for bit and whatever max_rows is; align_phonemes_long / align_words_long are asr_logprobs_long +
ctc_align_long + the host functions by hand, and equal align_phonemes / align_words inside those calls' limits; align_wav_long is the
segment chain by hand and equals align_wav on a short clip; scripts/align.py --long runs end to end on a 40 s clip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from smalltts_amd.api import HOP_SIZE, SmallTTS, token_groups, word_times
from smalltts_amd.plans import CTC_HOP, group_confidence, long_windows, speaking_rate
from smalltts_amd.weights import CodecSpec

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 225
IDS = [41, 45, 14, 77, 120, 1, 14, 33, 41, 14, 41, 41, 52, 14, 60, 61, 62, 63, 14, 70, 71, 1, 14, 80, 81] * 6     # 150 tokens


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(SEED, parts=("dit", "decoder", "encoder", "asr"), codec_spec=SPEC)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def tts(eng):
    return SmallTTS(engine=eng, seed=1, recogniser=True)


@pytest.fixture(scope="module")
def latents():
    return np.random.default_rng(5).standard_normal((406, 64)).astype(F32)


def stitched(eng, x):
    """asr_logprobs of every window alone, stitched in numpy by the window table"""
    N = x.shape[0]
    starts, cuts, src = long_windows(N)
    out = np.zeros((4 * N, 198), F32)
    for w, a in enumerate(starts):
        n = min(W, N)
        lp = eng.asr_logprobs(torch.from_numpy(x[a:a + n][None].copy()).to(eng.device), [n]).cpu().numpy()[0]
        for f in np.flatnonzero(src == w):
            out[4 * f:4 * f + 4] = lp[4 * (f - a):4 * (f - a) + 4]
    return out


@pytest.mark.parametrize("N", [226, 405, 406])
def test_asr_logprobs_long_is_the_windows_by_hand(eng, latents, N):
    x = latents[:N]
    got = eng.asr_logprobs_long(torch.from_numpy(x).to(eng.device))
    assert got.shape == (4 * N, 198) and got.dtype == torch.float32 and got.is_contiguous()
    assert got.cpu().numpy().tobytes() == stitched(eng, x).tobytes()
    if N == 406:
        few = eng.asr_logprobs_long(torch.from_numpy(x).to(eng.device), max_rows=2)        # three windows in two turns
        assert few.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()


def test_asr_logprobs_long_of_a_short_recording_is_asr_logprobs(eng, latents):
    for N in (1, 40, 225):
        x = torch.from_numpy(latents[:N]).to(eng.device)
        assert eng.asr_logprobs_long(x).cpu().numpy().tobytes() == eng.asr_logprobs(x[None], [N])[0].cpu().numpy().tobytes()
    for bad in (latents[:5], torch.zeros(5, 63, device=eng.device), torch.zeros(1, 5, 64, device=eng.device),
                torch.zeros(16385, 64, device=eng.device)):
        with pytest.raises(ValueError, match="asr_logprobs_long"):
            eng.asr_logprobs_long(bad)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_rows"):
            eng.asr_logprobs_long(torch.zeros(5, 64, device=eng.device), max_rows=bad)


def test_align_phonemes_long_and_words_long_are_the_chain_by_hand(tts, eng, latents):
    N = 406
    logp = eng.asr_logprobs_long(torch.from_numpy(latents).to(eng.device))
    tab = torch.tensor([IDS], dtype=torch.int32, device=eng.device)
    spans, tok_logp, score = (o.cpu().numpy() for o in eng.ctc_align_long(logp[None], [4 * N], tab, [0], [len(IDS)]))
    sp, tl, sc = tts.align_phonemes_long(latents, IDS)
    assert sp.shape == (len(IDS), 2) and sp.dtype == np.int32 and tl.shape == (len(IDS),) and tl.dtype == F32 and isinstance(sc, float)
    assert np.array_equal(sp, spans[0]) and tl.tobytes() == tok_logp[0].tobytes() and F32(sc).tobytes() == score[0].tobytes()
    assert np.isfinite(sc) and (sp >= 0).all() and sp.max() < 4 * N and (np.diff(sp.reshape(-1)) >= 0).all()
    groups = token_groups(IDS)
    times = word_times(groups, spans[0], 4 * N, token0=0, hop=CTC_HOP)
    conf = group_confidence(groups, spans[0], tok_logp[0], token0=0)
    words = tts.align_words_long(torch.from_numpy(latents), IDS)             # a CPU tensor is taken like an array
    assert words == [(i, kind, g[1], s, e, c) for (i, kind, s, e), g, c in zip(times, groups, conf)]
    assert all(0 <= s <= e <= HOP_SIZE * N and c <= 0.0 for _i, _k, _ph, s, e, c in words)
    w2, s2 = tts.align_words_long(latents, IDS, return_spans=True)
    assert w2 == words and np.array_equal(s2, sp)
    rate, seconds = speaking_rate(s2)
    assert 0 < seconds <= N * HOP_SIZE / 24000 and rate == len(IDS) / seconds
    for bad in (latents[None], latents[:, :63], np.zeros((0, 64), F32)):
        with pytest.raises(ValueError, match="align_words_long"):
            tts.align_words_long(bad, IDS)
    with pytest.raises(ValueError, match="16383 tokens"):
        tts.align_phonemes_long(latents, [5] * 16384)


def test_inside_the_old_limits_the_long_calls_equal_the_short_ones(tts, latents):
    for N, ids in ((40, IDS[:20]), (225, IDS + IDS[:48])):               # the second: 225 frames and 198 ids, both limits
        x = latents[:N]
        assert tts.align_words_long(x, ids) == tts.align_words([x], [ids])[0]
        a, b = tts.align_phonemes_long(x, ids), tts.align_phonemes([x], [ids])[0]
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    off = tts.align_words_long(latents[:1], [50, 50, 50, 50])            # not aligned: the group collapses
    assert off == tts.align_words([latents[:1]], [[50, 50, 50, 50]])[0] and off[0][3:] == (0, 0, float("-inf"))


def _clip(seconds, sr=16000):
    t = np.arange(int(seconds * sr)) / sr
    return (0.4 * np.sin(2 * np.pi * 330 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t))).astype(F32)


def test_align_wav_long_is_the_segment_chain_by_hand(tts, eng):
    sr = 16000
    clip = _clip(20 * HOP_SIZE / 24000 + 0.01, sr)                        # 20 whole hops and a little
    ids = IDS[:30]
    got = tts.align_wav_long(clip, sr, ids, enc_frames=8, enc_context=2)
    y = eng.resample(clip, sr, 24000)
    assert int(y.numel()) // HOP_SIZE == 20
    seg = lambda f0, f1: eng.codec_encode(y[f0 * HOP_SIZE:f1 * HOP_SIZE].reshape(1, 1, -1))[0]
    lat = torch.cat([seg(0, 8), seg(6, 16)[2:], seg(14, 20)[2:]])
    assert lat.shape == (20, 64)
    assert tts.encode_wav_long(y, 8, 2).cpu().numpy().tobytes() == lat.cpu().numpy().tobytes()
    assert got == tts.align_words_long(lat, ids)
    assert got and all(0 <= s <= e <= 20 * HOP_SIZE for _i, _k, _ph, s, e, _c in got)
    assert tts.encode_wav_long(y, 20, 2).cpu().numpy().tobytes() == seg(0, 20).cpu().numpy().tobytes()  # at most enc_frames: one encode
    assert got == tts.align_wav_long(clip[None, :], sr, ids, enc_frames=8, enc_context=2)              # (1, S) is mono too
    with pytest.raises(ValueError, match="shorter than one codec hop"):
        tts.align_wav_long(clip[:1000], sr, ids)
    with pytest.raises(ValueError, match="enc_frames"):
        tts.align_wav_long(clip, sr, ids, enc_frames=0)


def test_align_wav_long_on_a_short_clip_is_align_wav(tts):
    clip = _clip(1.0)
    ids = IDS[:6]
    assert tts.align_wav_long(clip, 16000, ids) == tts.align_wav(clip, 16000, ids)
    with pytest.raises(ValueError, match="align_wav"):                   # the old call keeps its limit
        tts.align_wav(np.zeros(31 * 8000, F32), 8000, ids)


def test_align_cli_long_end_to_end_on_40_seconds(tmp_path):
    from smalltts_amd.audio import write_wav_pcm16
    sr = 8000
    write_wav_pcm16(str(tmp_path / "rec.wav"), _clip(40.0, sr), sr)
    words, srt = tmp_path / "out" / "words.json", tmp_path / "out" / "words.srt"
    toks = ",".join(str(t) for t in IDS)
    base = [sys.executable, "-m", "smalltts_amd.scripts.align", "--weights", "synthetic:3"]
    r = subprocess.run(base + ["--long", "--wav", str(tmp_path / "rec.wav"), "--text", "unused", "--tokens", toks, "--words", str(words),
                               "--srt", str(srt)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(words.read_text(encoding="utf-8"))
    assert sorted(js) == ["speaking_rate", "words"] and sorted(js["speaking_rate"]) == ["speech_seconds", "tokens_per_second"]
    n_groups = len(token_groups(IDS))
    assert f"{n_groups} word groups" in r.stdout and len(js["words"]) == n_groups
    assert 0 < js["speaking_rate"]["speech_seconds"] <= 40.0 and js["speaking_rate"]["tokens_per_second"] > 0
    end = 40 * 24000
    assert all(0 <= w["start"] <= w["end"] <= end and w["start"] % 800 == 0 for w in js["words"])
    starts = [w["start"] for w in js["words"]]
    assert starts == sorted(starts)
    assert srt.read_text(encoding="utf-8").count("-->") == n_groups
