"""GPU: the alignment calls of the Python API on synthetic weights with the recogniser part: align_phonemes is
engine.asr_logprobs + engine.ctc_align run by hand, align_words is word_times and group_confidence of those spans, align_wav is the
resampler, the codec encoder and align_words by hand, realign swaps a take's spans for the CTC spans // 4 and leaves its audio alone,
scripts/align.py runs end to end in both modes, and without the recogniser every call raises ValueError."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from smalltts_amd.api import HOP_SIZE, Encoder, Piece, SmallTTS, frames_of_groups, load_take, save_take, token_groups, word_times
from smalltts_amd.plans import CTC_HOP, codec_spans, group_confidence
from smalltts_amd.weights import CodecSpec

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# words, a space (14), a punctuation mark (1), behind a prefix of two tokens
TOKS = [[50, 60, 41, 45, 14, 77, 120, 1], [9, 9, 33, 41, 14, 41, 41, 52, 14, 60, 61, 62, 63, 14, 70, 71, 1, 14, 80, 81]]
PRE = [2, 2]
NS = [7, 40]


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
    g = np.random.default_rng(5)
    x = np.zeros((2, max(NS), 64), F32)
    for b, n in enumerate(NS):
        x[b, :n] = g.standard_normal((n, 64))
    return x


def by_hand(eng, x, ns, toks, pre):
    P = max(len(t) for t in toks)
    tab = np.zeros((len(toks), P), np.int32)
    for b, t in enumerate(toks):
        tab[b, :len(t)] = t
    logp = eng.asr_logprobs(torch.from_numpy(x).to(eng.device), ns)
    spans, tok_logp, score = eng.ctc_align(logp, [4 * n for n in ns], torch.from_numpy(tab).to(eng.device), pre, [len(t) for t in toks])
    torch.cuda.synchronize()
    return spans.cpu().numpy(), tok_logp.cpu().numpy(), score.cpu().numpy()


def test_align_phonemes_is_the_two_engine_calls_by_hand(tts, eng, latents):
    spans, tok_logp, score = by_hand(eng, latents, NS, TOKS, PRE)
    rows = tts.align_phonemes(latents, TOKS, lengths=NS, prefix_lens=PRE)
    assert len(rows) == 2
    for b, (sp, tl, sc) in enumerate(rows):
        L = len(TOKS[b])
        assert sp.shape == (L, 2) and sp.dtype == np.int32 and tl.shape == (L,) and tl.dtype == F32 and isinstance(sc, float)
        assert np.array_equal(sp, spans[b, :L]) and tl.tobytes() == tok_logp[b, :L].tobytes() and F32(sc).tobytes() == score[b].tobytes()
        assert np.isfinite(sc) and (sp[:PRE[b]] == -1).all() and (sp[PRE[b]:] >= 0).all() and sp.max() < 4 * NS[b]
        assert (np.diff(sp[PRE[b]:].reshape(-1)) >= 0).all()                 # monotone: first <= last < the next token's first
    again = tts.align_phonemes([latents[0, :NS[0]], latents[1, :NS[1]]], TOKS, prefix_lens=PRE)   # rows carry their own lengths
    assert all(np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] for a, b in zip(again, rows))
    short = tts.align_phonemes(latents[:1, :1], [[50, 50, 50, 50]])              # four equal labels need seven frames, the row has four
    assert np.isneginf(short[0][2]) and (short[0][0] == -1).all() and not short[0][1].any()


def test_align_words_is_word_times_of_those_spans(tts, eng, latents):
    spans, tok_logp, _score = by_hand(eng, latents, NS, TOKS, PRE)
    words = tts.align_words(latents, TOKS, lengths=NS, prefix_lens=PRE)
    for b in range(2):
        groups = token_groups(TOKS[b][PRE[b]:])
        times = word_times(groups, spans[b], 4 * NS[b], token0=PRE[b], hop=CTC_HOP)
        conf = group_confidence(groups, spans[b], tok_logp[b], token0=PRE[b])
        assert words[b] == [(i, kind, g[1], s, e, c) for (i, kind, s, e), g, c in zip(times, groups, conf)]
        assert len(words[b]) == len(groups) > 0
        assert all(0 <= s < e <= HOP_SIZE * NS[b] and s % 800 == 0 and e % 800 == 0 and c <= 0.0 for _i, _k, _ph, s, e, c in words[b])
        assert [w[3] for w in words[b]] == sorted(w[3] for w in words[b])
    off = tts.align_words(latents[:1, :1], [[50, 50, 50, 50]])[0]                # not aligned: the group collapses
    assert off == [(0, "word", off[0][2], 0, 0, float("-inf"))]


def test_align_wav_is_the_chain_by_hand(tts, eng):
    sr = 16000
    t = np.arange(sr) / sr                                                   # 1 s: 24000 samples, 7 whole hops
    clip = (0.4 * np.sin(2 * np.pi * 330 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t))).astype(F32)
    ids = TOKS[0][PRE[0]:]
    got = tts.align_wav(clip, sr, ids)
    y = eng.resample(clip, sr, 24000)
    lat = Encoder(engine=eng).encode_reference(y.reshape(1, 1, -1))
    assert lat.shape == (1, 7, 64)
    assert got == tts.align_words([lat[0].numpy()], [ids])[0]
    assert got and all(0 <= s <= e <= 7 * HOP_SIZE for _i, _k, _ph, s, e, _c in got)
    assert got == tts.align_wav(clip[None, :], sr, ids)                      # (1, S) is mono too
    with pytest.raises(ValueError, match="shorter than one codec hop"):
        tts.align_wav(clip[:1000], sr, ids)


def test_realign_swaps_the_spans_and_leaves_the_audio(tts, eng):
    g = np.random.default_rng(0)
    voice = tts.encode_voice(g.standard_normal((6, 64)).astype(F32))
    toks = [[41, 45, 14, 77, 120, 1], [33, 41, 14, 52, 60, 61, 14, 70, 1]]
    kw = dict(token_lists=toks, durations=[1.0, 2.0], seed=3, prefix_tokens=[9, 10])
    out, _words, pieces = tts.synthesize_long(voice, return_words=True, return_pieces=True, **kw)
    assert len(pieces) == 2 and all(p.prefix_len == 2 and p.spans is not None for p in pieces)
    new = tts.realign(pieces)
    rows = tts.align_phonemes([p.latents for p in pieces], [p.tokens for p in pieces], prefix_lens=[2, 2])
    for p, q, (sp, _tl, sc) in zip(pieces, new, rows):
        assert isinstance(q, Piece) and q.tokens == p.tokens and q.prefix_len == 2 and q.seed == p.seed and np.array_equal(q.latents, p.latents)
        assert np.isfinite(sc) and np.array_equal(q.spans, codec_spans(sp)) and q.spans.dtype == np.int32
        assert np.array_equal(q.spans[2:], sp[2:] // 4) and (q.spans[:2] == -1).all() and q.spans.max() < p.latents.shape[0]
        groups = token_groups(q.tokens[2:])
        f0, f1 = frames_of_groups(groups, q.spans, 0, len(groups), token0=2)
        assert 0 <= f0 < f1 <= p.latents.shape[0]
    assert np.array_equal(tts.render_long(new), tts.render_long(pieces))     # spans do not enter the audio
    assert np.array_equal(tts.render_long(new), out)
    # a piece that cannot be aligned (one frame = four recogniser frames for nine tokens) keeps its spans
    tiny = Piece(pieces[1].tokens, 0, pieces[1].latents[:1], 5, np.full((len(pieces[1].tokens), 2), 0, np.int32))
    kept = tts.realign([tiny, pieces[0]])
    assert np.array_equal(kept[0].spans, tiny.spans) and np.array_equal(kept[1].spans, new[0].spans)


def test_align_cli_end_to_end_in_both_modes(tmp_path):
    from smalltts_amd.audio import write_wav_pcm16
    sr = 16000
    t = np.arange(int(1.2 * sr)) / sr
    write_wav_pcm16(str(tmp_path / "rec.wav"), 0.5 * np.sin(2 * np.pi * 440 * t), sr)
    words, srt = tmp_path / "out" / "words.json", tmp_path / "out" / "words.srt"
    base = [sys.executable, "-m", "smalltts_amd.scripts.align", "--weights", "synthetic:3"]
    r = subprocess.run(base + ["--wav", str(tmp_path / "rec.wav"), "--text", "unused", "--tokens", "41,45,14,77,120,1", "--words", str(words),
                               "--srt", str(srt)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert str(words) in r.stdout and "3 word groups" in r.stdout
    js = json.loads(words.read_text(encoding="utf-8"))
    assert [w["kind"] for w in js] == ["word", "word", "punct"] and [w["index"] for w in js] == [0, 1, 2]
    assert all(0 <= w["start"] < w["end"] <= 9 * HOP_SIZE and w["start"] % 800 == 0 and w["confidence"] <= 0 for w in js)
    assert srt.read_text(encoding="utf-8").count("-->") == 3
    # --take: a take of this engine's pieces, written, aligned again by the script, read back
    g = np.random.default_rng(1)
    pieces = [Piece([9, 41, 45, 14, 77], 1, g.standard_normal((6, 64)).astype(F32), 4, np.zeros((5, 2), np.int32)),
              Piece([33, 52, 1], 0, g.standard_normal((3, 64)).astype(F32), 5)]
    save_take(str(tmp_path / "in.npz"), pieces, gap_ms=90.0, trim=True, level_dbfs=-20.0)
    r = subprocess.run(base + ["--take", str(tmp_path / "in.npz"), "--out-take", str(tmp_path / "o" / "out.npz")], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got, join = load_take(str(tmp_path / "o" / "out.npz"))
    assert join == load_take(str(tmp_path / "in.npz"))[1] and join["gap_ms"] == 90.0 and join["trim"] is True
    for p, q in zip(pieces, got):
        assert q.tokens == p.tokens and q.prefix_len == p.prefix_len and q.seed == p.seed and np.array_equal(q.latents, p.latents)
        assert q.spans is not None and (q.spans[:p.prefix_len] == -1).all() and (q.spans[p.prefix_len:] >= 0).all()
        assert q.spans.max() < p.latents.shape[0]


def test_without_the_recogniser_every_call_raises(eng):
    from smalltts_amd.engine import HipEngine
    bare = HipEngine(0, "bf16x3")
    bare.load_synthetic(SEED, parts=("dit", "decoder", "encoder"), codec_spec=SPEC)
    bare.finalize()
    t2 = SmallTTS(engine=bare, seed=1)
    x = np.zeros((1, 4, 64), F32)
    for call in (lambda: t2.align_phonemes(x, [[3, 4]]), lambda: t2.align_words(x, [[3, 4]]),
                 lambda: t2.align_wav(np.zeros(24000, F32), 24000, [3, 4]), lambda: t2.realign([Piece([3, 4], 0, x[0], 1)])):
        with pytest.raises(ValueError, match="recogniser"):
            call()
