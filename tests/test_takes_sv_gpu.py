"""GPU: Takes(sv=): synthesize_batch(3 rows, takes=Takes(3, sv=w)) against the same nine rows run by hand through the public
calls: cos is speaker_similarity of the hand rows bit for bit, total' = total + sv * (1 - cos) is reproduced by numpy float32 in that
order (behind the CTC term where that is on), winners, latents and audio are those of the hand-picked rows; a weight and a seed at
which the winner differs from the sv = 0 winner; sv = 0 is the call of today; every case that cannot be scored is a ValueError."""
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
REFS = (6, 9, 7)                                  # reference frames of the three voices (6: the shortest with an embedding)
SEEDS = [21, 22, 23]
K = 3
SV = 2.0
# CHOSEN, not derived: random weights give cosines near 0.96 that differ in the second decimal, so the term moves a winner only where
# two totals are close.  (DIFF_W, DIFF_SEED): the first pair among the weights 4, 16, 64 and the base seeds 0 .. 31 (rows seeded
# DIFF_SEED, DIFF_SEED + 1, DIFF_SEED + 2) at which it does, found on an MI355X by tools/sv_bench.py --find-seed
DIFF_W, DIFF_SEED = 4.0, 0


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(SEED, parts=("dit", "decoder", "encoder", "asr", "sv"), codec_spec=SPEC)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def tts(eng):
    return SmallTTS(engine=eng, seed=1, recogniser=True, verifier=True)


@pytest.fixture(scope="module")
def refs():
    g = np.random.default_rng(0)
    return [g.standard_normal((r, 64)).astype(np.float32) for r in REFS]


@pytest.fixture(scope="module")
def voices(tts, refs):
    return [tts.encode_voice(r) for r in refs]


def by_hand(tts, voices, seeds, w, ctc=0.0, refs=None):
    """The nine sampler rows through the public calls -> (latents of the 9 rows, cos (3, K), total' (3, K), winners, winners without
    the term).  refs: the reference latents instead of the voices."""
    rows = [g for g in range(3) for _ in range(K)]
    who = dict(voices=[voices[g] for g in rows]) if refs is None else {}
    _audio, lat = tts.synthesize_batch(None if refs is None else [refs[g] for g in rows], [TOKS[g] for g in rows], None,
                                       frames=[NS[g] for g in rows], seeds=[take_seed(seeds[g], k) for g in range(3) for k in range(K)],
                                       return_latents=True, **who)
    who = dict(voices=voices) if refs is None else {}
    plain = tts.synthesize_batch(None if refs is None else refs, TOKS, None, frames=NS, seeds=seeds, takes=Takes(K, ctc=ctc),
                                 return_takes=True, **who)[-1]
    tot0 = np.stack([t[2] for t in plain]).astype(F32)                       # (with ctc: the CTC term is in it, tests/test_takes_ctc_gpu.py)
    cos = np.asarray([tts.speaker_similarity([lat[g * K + k] for k in range(K)], voices[g] if refs is None else refs[g])
                      for g in range(3)], F32)
    tot = tot0 + (F32(1.0) - cos) * F32(w)                                   # numpy float32, the stated order
    assert tot.dtype == F32 and cos.dtype == F32
    key = np.where(np.isnan(tot), np.inf, tot)
    return lat, cos, tot, key.argmin(axis=1), np.asarray([t[0] for t in plain])


@pytest.mark.parametrize("ctc", [0.0, 1.0])
def test_takes_with_the_speaker_term_equal_the_rows_by_hand(tts, eng, voices, ctc):
    lat9, cos, tot, win, _ = by_hand(tts, voices, SEEDS, SV, ctc)
    tk = Takes(K, ctc=ctc, sv=SV)
    rows, lat, taken = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=SEEDS, takes=tk, return_takes=True,
                                            return_latents=True)
    print(f"\n[takes sv, ctc {ctc}] winners {win.tolist()} cos {cos.tolist()} totals {tot.tolist()}")
    assert np.isfinite(cos).all() and (np.abs(cos) < 1.0).all() and len(set(cos.reshape(-1).tolist())) == 3 * K
    pad = np.zeros((3, max(NS), 64), F32)
    for g in range(3):
        assert len(taken[g]) == (6 if ctc else 5)                           # ..., nll where the CTC term is on, cos last
        k, seed, t, ft, c = taken[g][0], taken[g][1], taken[g][2], taken[g][3], taken[g][-1]
        assert k == int(win[g]) and seed == take_seed(SEEDS[g], k) and ft.shape == (K, 4)
        assert c.astype(F32).tobytes() == cos[g].tobytes()                  # speaker_similarity of the hand rows, bit for bit
        assert t.astype(F32).tobytes() == tot[g].tobytes()                  # total + (1 - cos) * sv in numpy float32
        assert lat[g].tobytes() == lat9[g * K + k].tobytes()
        pad[g, : NS[g]] = lat[g]
    dec = eng.codec_decode(torch.from_numpy(pad).to(eng.device)).cpu().numpy()
    for g in range(3):
        assert rows[g].shape == (1, HOP_SIZE * NS[g]) and rows[g].tobytes() == np.ascontiguousarray(dec[g, :, : HOP_SIZE * NS[g]]).tobytes()
    again = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=SEEDS, takes=tk, return_latents=True)
    assert all(again[0][g].tobytes() == rows[g].tobytes() and again[1][g].tobytes() == lat[g].tobytes() for g in range(3))


def test_without_a_voice_the_reference_is_embedded_in_the_same_call(tts, voices, refs):
    lat9, cos, tot, win, _ = by_hand(tts, voices, SEEDS, SV, refs=refs)
    _rows, lat, taken = tts.synthesize_batch(refs, TOKS, None, frames=NS, seeds=SEEDS, takes=Takes(K, sv=SV), return_takes=True,
                                             return_latents=True)
    for g in range(3):
        assert taken[g][0] == int(win[g]) and taken[g][-1].astype(F32).tobytes() == cos[g].tobytes()
        assert taken[g][2].astype(F32).tobytes() == tot[g].tobytes() and lat[g].tobytes() == lat9[g * K + int(win[g])].tobytes()


def test_a_weight_and_a_seed_at_which_the_speaker_term_changes_the_winner(tts, voices):
    seeds = [DIFF_SEED, DIFF_SEED + 1, DIFF_SEED + 2]
    lat9, cos, tot, win, win0 = by_hand(tts, voices, seeds, DIFF_W)
    print(f"\n[takes sv] sv {DIFF_W} seed {DIFF_SEED}: winners without the term {win0.tolist()}, with it {win.tolist()}")
    assert (win != win0).any()
    _rows, lat, taken = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=seeds, takes=Takes(K, sv=DIFF_W),
                                             return_takes=True, return_latents=True)
    assert [t[0] for t in taken] == win.tolist()
    assert all(lat[g].tobytes() == lat9[g * K + int(win[g])].tobytes() for g in range(3))


def test_sv_zero_is_the_call_of_today(tts, voices):
    kw = dict(frames=NS, voices=voices, seeds=SEEDS, return_takes=True, return_latents=True)
    a = tts.synthesize_batch(None, TOKS, None, takes=Takes(K), **kw)
    b = tts.synthesize_batch(None, TOKS, None, takes=Takes(K, sv=0.0), **kw)
    c = tts.synthesize_batch(None, TOKS, None, takes=K, **kw)
    for g in range(3):
        assert a[0][g].tobytes() == b[0][g].tobytes() == c[0][g].tobytes() and a[1][g].tobytes() == b[1][g].tobytes() == c[1][g].tobytes()
        assert len(a[2][g]) == len(b[2][g]) == len(c[2][g]) == 4            # no cosines in the report
        assert a[2][g][:2] == b[2][g][:2] == c[2][g][:2] and a[2][g][2].tobytes() == b[2][g][2].tobytes() == c[2][g][2].tobytes()


def test_synthesize_long_and_respeak_pass_the_term_through(tts, voices):
    kw = dict(token_lists=TOKS, durations=[n / 7.5 for n in NS], seed=5, return_takes=True)
    wave0, taken0 = tts.synthesize_long(voices[1], takes=K, **kw)
    wave, taken = tts.synthesize_long(voices[1], takes=Takes(K, sv=SV), **kw)
    assert wave.shape[1] > 0 and len(taken) == 3 and all(len(t) == 5 and t[-1].shape == (K,) for t in taken) and all(len(t) == 4 for t in taken0)
    for t0, t in zip(taken0, taken):
        want = t0[2].astype(F32) + (F32(1.0) - t[-1].astype(F32)) * F32(SV)
        assert t[2].astype(F32).tobytes() == want.tobytes()
    _a, lat = tts.synthesize_batch(None, TOKS[:1], None, frames=NS[:1], voices=voices[:1], seeds=[3], return_latents=True)
    res = tts.respeak(TOKS[0], lat[0], (2, 6), voice=voices[0], seed=4, takes=Takes(2, sv=SV), return_takes=True)
    assert len(res[-1]) == 5 and res[-1][-1].shape == (2,)
    with pytest.raises(ValueError, match="frames in every row"):
        tts.synthesize_long(voices[1], token_lists=TOKS, durations=[1.2, 0.5, 1.2], takes=Takes(K, sv=SV))


def test_every_case_that_cannot_be_scored_is_a_value_error(tts, eng, voices, refs):
    from smalltts_amd.engine import HipEngine
    tk = Takes(2, sv=1.0)
    with pytest.raises(ValueError, match="frames in every row"):            # a row under 6 frames
        tts.synthesize_batch(None, TOKS[:2], None, frames=[9, 5], voices=voices[:2], takes=tk)
    short = tts.encode_voice(refs[1][:5])                                   # a reference without an embedding
    assert short.speaker is None and voices[0].speaker is not None and tuple(voices[0].speaker.shape) == (192,)
    with pytest.raises(ValueError, match="speaker embedding"):
        tts.synthesize_batch(None, TOKS[:1], None, frames=NS[:1], voices=[short], takes=tk)
    with pytest.raises(ValueError, match="reference frames"):
        tts.synthesize_batch([refs[1][:5]], TOKS[:1], None, frames=NS[:1], takes=tk)
    with pytest.raises(ValueError, match="repair"):
        tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, takes=tk, repair=Repair(1))
    assert len(tts.synthesize_batch(None, TOKS[:1], None, frames=NS[:1], voices=[short], takes=Takes(2))) == 1   # sv = 0: as ever
    bare = HipEngine(0, "bf16x3")                                           # an engine without the part
    bare.load_synthetic(SEED, parts=("dit", "decoder", "encoder"), codec_spec=SPEC)
    bare.finalize()
    t2 = SmallTTS(engine=bare, seed=1)
    v2 = [t2.encode_voice(refs[1])]
    assert v2[0].speaker is None
    with pytest.raises(ValueError, match="verifier"):
        t2.synthesize_batch(None, TOKS[:1], None, frames=NS[:1], voices=v2, takes=tk)
    with pytest.raises(ValueError, match="verifier"):
        t2.speaker_embedding(np.zeros((1, 8, 64), F32))
    with pytest.raises(ValueError, match="verifier"):
        t2.speaker_similarity(np.zeros((1, 8, 64), F32), refs[1])
    with pytest.raises(RuntimeError, match="verifier"):
        SmallTTS(engine=bare, verifier=True)
    with pytest.raises(ValueError, match="another engine"):
        tts.speaker_similarity(np.zeros((1, 8, 64), F32), v2[0])


def test_speaker_embedding_and_similarity_public_calls(tts, eng, voices, refs):
    g = np.random.default_rng(3)
    x = g.standard_normal((2, 12, 64)).astype(F32)
    emb = tts.speaker_embedding(x, lengths=[12, 7])
    assert emb.shape == (2, 192) and emb.dtype == F32
    dev = eng.sv_embed(torch.from_numpy(x).to(eng.device), [12, 7])
    assert emb.tobytes() == dev.cpu().numpy().tobytes()
    assert tts.speaker_embedding([x[0], x[1, :7]]).tobytes() == emb.tobytes()        # a list of rows carries its own lengths
    assert voices[1].speaker.cpu().numpy().tobytes() == tts.speaker_embedding(refs[1][None])[0].tobytes()
    sim = tts.speaker_similarity(x, voices[1], lengths=[12, 7])
    assert sim == tts.speaker_similarity(x, refs[1], lengths=[12, 7]) == tts.speaker_similarity(x, [refs[1], refs[1]], lengths=[12, 7])
    want = eng.sv_cosine(dev, voices[1].speaker[None].contiguous(), 2).cpu().numpy()
    assert np.asarray(sim, F32).tobytes() == want.tobytes() and all(-1.0 <= v <= 1.0 for v in sim)
    assert abs(tts.speaker_similarity(refs[1][None], voices[1])[0] - 1.0) <= 200 * 2.0 ** -24
    for bad, kw in ((x, dict(lengths=[12, 5])), (np.zeros((1, 226, 64), F32), {}), ([x[0][:5]], {}), (np.zeros((65, 6, 64), F32), {})):
        with pytest.raises(ValueError):
            tts.speaker_embedding(bad, **kw)
    with pytest.raises(ValueError):
        tts.speaker_similarity(x, refs[1][:5])
    with pytest.raises(ValueError, match="one per row"):
        tts.speaker_similarity(x, [refs[1]] * 3)
    assert tts.speaker_embedding(np.zeros((1, 300, 64), F32), lengths=[225]).shape == (1, 192)   # padding behind the longest row is cut
