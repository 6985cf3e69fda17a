"""GPU: what a synthesis call returns after the fp16 range guard made it run again.

The guard (engine.check_fp16_range) fires after a batch whose fp16 operands clamped: the site is demoted to split-bf16 and the
call enqueues the same work once more.  Whatever the call returns next to the audio — latents, speech windows, word timings, raw
alignment, long-form segments and Pieces — must then belong to the SECOND run.  Each scenario makes the same call twice on one
engine whose DiT weights are known to clamp (test_range_guard_gpu._outlier_dit_weights): call A on the fresh engine warns and
re-runs, call B runs once on the now demoted engine with the same seeds, and every element A returned equals B's bit for bit.
Demotion is sticky, so every scenario builds its own engine.

Calls that put batches in flight re-run under the caller's tuning (SmallTTS._run_in_flight), so those scenarios set throughput
tuning first: A's re-run and B's first pass then run the same kernels.
"""
import warnings

import numpy as np
import pytest

from smalltts_amd.api import Endpointing, Piece, SmallTTS
from smalltts_amd.weights import CodecSpec
from tests.test_range_guard_gpu import SEED, _outlier_dit_weights

pytestmark = pytest.mark.gpu

TINY = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1,) * 7)
FRAMES, TOKENS, VOICE_FRAMES = (40, 33), (12, 9), 10
_rng = np.random.default_rng(3)
REF = _rng.standard_normal((VOICE_FRAMES, 64)).astype(np.float32)
REF[:, [3, 17, 40]] *= 20.0
TOKS = [[int(t) for t in _rng.integers(1, 198, TOKENS[i % 2])] for i in range(4)]   # 12, 9, 12, 9 tokens
TRIM = Endpointing(level_dbfs=-20)


def _guard(rec):
    return [str(r.message) for r in rec if "fp16 range guard" in str(r.message)]


def _same(a, b, where="result"):
    """Bit-for-bit equality of two results: tuples / lists element by element, Pieces field by field, arrays by array_equal."""
    if isinstance(a, Piece):
        assert isinstance(b, Piece), where
        for f in Piece.__slots__:
            _same(getattr(a, f), getattr(b, f), f"{where}.{f}")
    elif isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), where
        assert a.dtype.kind != "f" or np.isfinite(a).all(), where
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


def _twice(call, tuning=None):
    """call(tts, voice) on a fresh engine (A: the guard fires, the call runs again) and once more on the same engine (B: silent);
    -> A's result, after it has been held to B's."""
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0)
    try:
        eng.load_state_dict(_outlier_dit_weights(factor_ff=400.0, w2_div=400.0 * 400.0))
        eng.load_synthetic(SEED, parts=("decoder",), codec_spec=TINY)
        eng.finalize()
        if tuning is not None:
            eng.set_tuning(tuning)
        voice = SmallTTS(engine=eng, seed=1).encode_voice(REF)
        print(f"\n[re-run] clamps while the voice was encoded: {eng.saturations(reset=True)}")
        results = []
        for name in "AB":
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                results.append(call(SmallTTS(engine=eng, seed=1), voice))
            msgs = _guard(rec)
            print(f"[re-run] call {name}: {msgs}")
            if name == "A":   # without the re-run the scenario shows nothing
                assert any("dit_block" in m for m in msgs), msgs
            else:
                assert not msgs, msgs
        _same(results[0], results[1])
        return results[0]
    finally:
        eng.close()


def test_batch_with_trim_align_latents_and_raw_alignment():
    def call(tts, voice):
        return tts.synthesize_batch(None, TOKS[:2], None, frames=list(FRAMES), voices=[voice] * 2, seeds=[11, 12], trim=TRIM,
                                    align=True, return_latents=True, return_alignment=True)
    outs, lats, words, raw = _twice(call)
    assert len(outs) == len(lats) == len(words) == len(raw) == 2
    assert [l.shape for l in lats] == [(n, 64) for n in FRAMES]
    assert [(m.shape, s.shape) for m, s in raw] == [((n, p), (p, 2)) for n, p in zip(FRAMES, TOKENS)]


def test_plain_batch_with_ref_latents():
    def call(tts, voice):
        return tts.synthesize_batch([REF, REF[:7]], TOKS[:2], None, frames=list(FRAMES), seeds=[11, 12], return_latents=True)
    outs, lats = _twice(call)
    assert [o.shape for o in outs] == [(1, 3200 * n) for n in FRAMES]
    assert [l.shape for l in lats] == [(n, 64) for n in FRAMES]


def test_batches_in_flight():
    durs = [(n + 0.5) / 7.5 for n in FRAMES]            # floor(d * 7.5) = n

    def call(tts, voice):
        return tts.synthesize_batches([([REF, REF[:7]], TOKS[:2], durs), ([REF[:7], REF], TOKS[2:], durs)], in_flight=2)
    outs = _twice(call, tuning="throughput")
    assert [[o.shape for o in batch] for batch in outs] == [[(1, 3200 * n) for n in FRAMES]] * 2


@pytest.mark.parametrize("trim", [TRIM, None], ids=["trim", "plain"])
def test_long_with_segments_words_and_pieces(trim):
    ns = [FRAMES[0], FRAMES[1], FRAMES[0]]

    def call(tts, voice):
        return tts.synthesize_long(voice, token_lists=TOKS[:3], durations=[(n + 0.5) / 7.5 for n in ns], seed=5, max_batch=2,
                                   in_flight=2, trim=trim, return_segments=True, return_words=True, return_pieces=True)
    wave, segs, words, pieces = _twice(call, tuning="throughput")
    assert len(segs) == len(pieces) == 3 and [p.latents.shape for p in pieces] == [(n, 64) for n in ns]
    assert all(p.spans is not None and p.spans.shape == (len(t), 2) for p, t in zip(pieces, TOKS))
    assert wave.shape[0] == 1 and all(0 <= off and off + n <= wave.shape[1] for off, n, _s, _g in segs)
