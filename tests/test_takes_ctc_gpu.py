"""GPU: Takes(ctc=): synthesize_batch(3 rows, takes=Takes(3, ctc=1.0)) against the same nine rows run by hand through the
public calls: nll is ctc_score of the hand rows bit for bit, total' = total + (ctc * nll) / tokens is reproduced by numpy float32 in that
order, winners, latents and audio are those of the hand-picked rows; a seed whose winner differs from the ctc = 0 winner; ctc = 0 is
the call of today; without the recogniser part a ValueError."""
import numpy as np
import pytest
import torch

from smalltts_amd.api import HOP_SIZE, Repair, SmallTTS, Takes, take_seed
from smalltts_amd.weights import CodecSpec

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
F32 = np.float32
TOKS = [[1, 2, 3, 4, 5, 6], [10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120], [7, 8, 9, 17, 18, 19, 27, 28, 29]]
NS = [9, 20, 14]
SEEDS = [21, 22, 23]
K = 3
CTC = 1.0
# a base seed (rows seeded DIFF_SEED, DIFF_SEED + 1, DIFF_SEED + 2) at which the CTC term changes a winner: found on an MI355X among the
# seeds 0 .. 31 by tools/asr_bench.py --find-seed (the first one that does)
DIFF_SEED = 0


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
def voices(tts):
    g = np.random.default_rng(0)
    return [tts.encode_voice(g.standard_normal((r, 64)).astype(np.float32)) for r in (5, 9, 7)]


def by_hand(tts, voices, seeds, ctc):
    """The nine sampler rows through the public calls -> (latents of the 9 rows, nll (3, K), total' (3, K), winners)."""
    rows = [g for g in range(3) for _ in range(K)]
    _audio, lat = tts.synthesize_batch(None, [TOKS[g] for g in rows], None, frames=[NS[g] for g in rows], voices=[voices[g] for g in rows],
                                       seeds=[take_seed(seeds[g], k) for g in range(3) for k in range(K)], return_latents=True)
    plain = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=seeds, takes=K, return_takes=True)[-1]
    tot0 = np.stack([t[2] for t in plain]).astype(F32)
    nll = np.asarray([v[0] for v in tts.ctc_score(lat, [TOKS[g] for g in rows])], F32).reshape(3, K)
    pw = np.asarray([[len(t)] * K for t in TOKS], F32)
    tot = tot0 + (F32(ctc) * nll) / pw                                      # numpy float32, the stated order
    assert tot.dtype == F32
    key = np.where(np.isnan(tot), np.inf, tot)
    return lat, nll, tot, key.argmin(axis=1), np.asarray([t[0] for t in plain])


def test_takes_with_the_ctc_term_equal_the_rows_by_hand(tts, eng, voices):
    lat9, nll, tot, win, _ = by_hand(tts, voices, SEEDS, CTC)
    rows, lat, taken = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=SEEDS, takes=Takes(K, ctc=CTC),
                                            return_takes=True, return_latents=True)
    print(f"\n[takes ctc] winners {win.tolist()} nll {nll.tolist()} totals {tot.tolist()}")
    assert np.isfinite(nll).all()
    pad = np.zeros((3, max(NS), 64), F32)
    for g in range(3):
        k, seed, t, ft, n = taken[g]
        assert k == int(win[g]) and seed == take_seed(SEEDS[g], k) and ft.shape == (K, 4)
        assert n.astype(F32).tobytes() == nll[g].tobytes()                  # ctc_score of the hand rows, bit for bit
        assert t.astype(F32).tobytes() == tot[g].tobytes()                  # total + (ctc * nll) / tokens in numpy float32
        assert lat[g].tobytes() == lat9[g * K + k].tobytes()
        pad[g, : NS[g]] = lat[g]
    dec = eng.codec_decode(torch.from_numpy(pad).to(eng.device)).cpu().numpy()
    for g in range(3):
        assert rows[g].shape == (1, HOP_SIZE * NS[g]) and rows[g].tobytes() == np.ascontiguousarray(dec[g, :, : HOP_SIZE * NS[g]]).tobytes()
    again = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=SEEDS, takes=Takes(K, ctc=CTC), return_latents=True)
    assert all(again[0][g].tobytes() == rows[g].tobytes() and again[1][g].tobytes() == lat[g].tobytes() for g in range(3))


def test_a_seed_at_which_the_ctc_term_changes_the_winner(tts, voices):
    seeds = [DIFF_SEED, DIFF_SEED + 1, DIFF_SEED + 2]
    lat9, nll, tot, win, win0 = by_hand(tts, voices, seeds, CTC)
    print(f"\n[takes ctc] seed {DIFF_SEED}: winners without the term {win0.tolist()}, with it {win.tolist()}")
    assert (win != win0).any()
    _rows, lat, taken = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=seeds, takes=Takes(K, ctc=CTC),
                                             return_takes=True, return_latents=True)
    assert [t[0] for t in taken] == win.tolist()
    assert all(lat[g].tobytes() == lat9[g * K + int(win[g])].tobytes() for g in range(3))


def test_ctc_zero_is_the_call_of_today(tts, voices):
    kw = dict(frames=NS, voices=voices, seeds=SEEDS, return_takes=True, return_latents=True)
    a = tts.synthesize_batch(None, TOKS, None, takes=Takes(K), **kw)
    b = tts.synthesize_batch(None, TOKS, None, takes=Takes(K, ctc=0.0), **kw)
    c = tts.synthesize_batch(None, TOKS, None, takes=K, **kw)
    for g in range(3):
        assert a[0][g].tobytes() == b[0][g].tobytes() == c[0][g].tobytes() and a[1][g].tobytes() == b[1][g].tobytes() == c[1][g].tobytes()
        assert len(a[2][g]) == len(b[2][g]) == len(c[2][g]) == 4            # no nll in the report
        assert a[2][g][:2] == b[2][g][:2] == c[2][g][:2] and a[2][g][2].tobytes() == b[2][g][2].tobytes() == c[2][g][2].tobytes()


def test_the_term_needs_the_recogniser_part_and_excludes_repair(tts, eng, voices):
    from smalltts_amd.engine import HipEngine
    bare = HipEngine(0, "bf16x3")
    bare.load_synthetic(SEED, parts=("dit", "decoder", "encoder"), codec_spec=SPEC)
    bare.finalize()
    t2 = SmallTTS(engine=bare, seed=1)
    v2 = [t2.encode_voice(np.zeros((4, 64), F32))]
    with pytest.raises(ValueError, match="recogniser"):
        t2.synthesize_batch(None, TOKS[:1], None, frames=NS[:1], voices=v2, takes=Takes(2, ctc=1.0))
    with pytest.raises(ValueError, match="recogniser"):
        t2.transcribe(np.zeros((1, 4, 64), F32))
    with pytest.raises(RuntimeError, match="recogniser"):
        SmallTTS(engine=bare, recogniser=True)
    with pytest.raises(ValueError, match="repair"):
        tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, takes=Takes(2, ctc=1.0), repair=Repair(1))
    assert len(t2.synthesize_batch(None, TOKS[:1], None, frames=NS[:1], voices=v2, takes=Takes(2))) == 1


def test_transcribe_and_ctc_score_public_calls(tts, eng):
    g = np.random.default_rng(3)
    x = g.standard_normal((2, 12, 64)).astype(F32)
    ids = tts.transcribe(x, lengths=[12, 5])
    logp = eng.asr_logprobs(torch.from_numpy(x).to(eng.device), [12, 5]).cpu().numpy()
    from tests.helpers import asr_ref as R
    assert ids == [R.greedy(logp[0], 48), R.greedy(logp[1], 20)]
    assert tts.transcribe([x[0], x[1, :5]]) == ids                          # a list of rows carries its own lengths
    sc = tts.ctc_score(x, [[3, 4, 5, 6], [9, 9, 7]], lengths=[12, 5], prefix_lens=[1, 0])
    assert all(np.isfinite(a) and b == pytest.approx(a / L, rel=1e-6) for (a, b), L in zip(sc, (3, 3)))
    want = R.ctc_nll(logp[0], 48, [4, 5, 6])
    assert abs(sc[0][0] - want) <= 4 * 48 * 2.0 ** -24 * max(1.0, abs(want))
    assert np.isposinf(tts.ctc_score(x, [[3], []], lengths=[0, 5])).all()
