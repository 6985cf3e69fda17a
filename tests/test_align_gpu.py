"""GPU: word timings from the DiT's text attention — the tap kernel through its hook against an fp64 softmax, a planted alignment,
the path kernel against the float32 restatement (tests/helpers/align_ref.py), the whole sampler path against the stage oracle, and the
public results on top (synthesize_batch(align=), synthesize_long(return_words=), the server's align=1).

Bars.  Tap kernel vs fp64, rel-L2 over mass, per operand format: the bars tests/test_kernels_gpu.py::test_attention holds the
attention OUTPUT to at the same format (bf16x3 3e-5, f16 1.5e-3, bf16 1.2e-2) — same images, same logits, a linear read-out of the
same probabilities.  Path kernel: spans and score equal the restatement exactly; the score lies within (N + P) 2^-24 score of the
float64 sum along the path ((N + P) fp32 additions of non-negative terms).  Whole path vs the oracle: not derivable (the error passes
through up to 12 blocks and 4 steps), so measured on both shapes and set at 4x the larger figure — see MASS_BARS."""
import http.client
import json
import threading

import numpy as np
import pytest
import torch

from oracle import dit_oracle as O
from smalltts_amd import server as S
from smalltts_amd.api import HOP_SIZE, Alignment, Endpointing, piece_seed, token_groups, word_times
from smalltts_amd.weights import CodecSpec
from tests.conftest import golden, rel_l2
from tests.helpers import align_ref as R

pytestmark = pytest.mark.gpu
TAP_BARS = {"bf16x3": 3e-5, "f16": 1.5e-3, "bf16": 1.2e-2}
# rel-L2 of sample(align=...)'s mass against the fp64 stage oracle (tests/helpers/align_ref.py sampler_text_mass), measured on an
# MI355X at the golden case_small shape and at the bench shape (8 x 75 frames, R = 15, P = 30), default selection (12 layers x 8 heads,
# last step):   bf16x3: small 2.548e-6, bench 2.804e-6        f16 (the default preset): small 1.597e-4, bench 1.627e-4
# bar = 4 x the larger figure of the preset (the margin is for other seeds, shapes and selections; the selection
# layers (0, 5, 11) x heads (1, 6) x steps (0, -1) measured 7.45e-6 at bf16x3 on the small shape)
MASS_BARS = {"bf16x3": 4 * 2.804e-6, "f16": 4 * 1.627e-4}
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def keng():
    """kernel hooks only: no weights"""
    from smalltts_amd.engine import HipEngine
    return HipEngine(0, "bf16x3")


# ---- the tap kernel through the hook -------------------------------------------------------------------------------------------------
def _attn_inputs(B, N, H, dh, rot, R_, P, seed0, tail):
    """the inputs and masks of tests/test_kernels_gpu.py::test_attention (seed0 = 20) / its many-tiles test (seed0 = 40)"""
    D = H * dh
    qkvg = _rand(B, N, 4 * D, seed=seed0)
    qw, kw = 1 + 0.2 * _rand(H, dh, seed=seed0 + 1), 1 + 0.2 * _rand(H, dh, seed=seed0 + 2)
    inv = 1.0 / (1e4 ** (torch.arange(0, rot, 2).float() / rot))
    rope = (torch.arange(max(N, 1)).float()[:, None] * inv[None]).repeat_interleave(2, -1).contiguous()
    ms = torch.ones(B, N, dtype=torch.bool); ms[-1, N - tail:] = False
    kr = vr = mr = None
    if R_:
        kr, vr = _rand(B, H, R_, dh, seed=seed0 + 3), _rand(B, H, R_, dh, seed=seed0 + 4)
        mr = torch.ones(B, R_, dtype=torch.bool); mr[0, (R_ // 2 if seed0 == 20 else 7):] = False      # a half-masked reference
    kt, vt = _rand(B, H, P, dh, seed=seed0 + 5), _rand(B, H, P, dh, seed=seed0 + 6)
    mt = torch.ones(B, P, dtype=torch.bool)
    if B > 1:
        mt[-1, :] = False                                                                                 # a fully masked text row
        mt[0, P // 3] = False                                                                             # ... and one masked column
    else:
        mt[0, P // 2:] = False                                                                            # (one row: half of its text)
    return qkvg, qw, kw, rope, kr, vr, kt, vt, ms, mr, mt


TAP_CASES = [(2, 75, 8, 120, 64, 15, 30, 20), (2, 130, 8, 120, 64, 70, 90, 20), (1, 5, 8, 120, 64, 3, 2, 20), (16, 75, 8, 120, 64, 15, 30, 20),
             (2, 40, 4, 128, 128, 0, 6, 20), (3, 21, 8, 64, 64, 0, 9, 20),
             (64, 75, 8, 120, 64, 15, 30, 40), (1, 300, 8, 120, 64, 150, 250, 40)]     # B = 64; Ktot = 700


@pytest.mark.parametrize("B,N,H,dh,rot,R_,P,seed0", TAP_CASES)
@pytest.mark.parametrize("fmt", ["bf16x3", "f16", "bf16"])
def test_text_mass_kernel_vs_fp64_softmax(keng, B, N, H, dh, rot, R_, P, seed0, fmt):
    qkvg, qw, kw, rope, kr, vr, kt, vt, ms, mr, mt = _attn_inputs(B, N, H, dh, rot, R_, P, seed0, N // 4 if seed0 == 20 else 7)
    ref = R.text_mass_fp64(qkvg, qw, kw, 1e-6, rope, rot, H, dh, kr, kt, ms, mr, mt).numpy()
    run = lambda: keng.test_attn_text_mass(qkvg, qw, kw, 1e-6, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt, fmt=fmt).cpu().numpy()
    got = run()
    assert got.shape == (B, N, P) and np.isfinite(got).all()
    # exact zeros: padded frames, masked text columns, the fully masked text row
    assert not got[~ms.numpy()].any() and not got.transpose(0, 2, 1)[~mt.numpy()].any() and (B == 1 or not got[-1].any())
    assert float(got.sum(-1).max()) <= 1.0 + 1e-6 and float(got.min()) >= 0.0
    assert got.any() and ref.any()
    err = rel_l2(got, ref)
    print(f"\n[text mass] B={B} N={N} H={H} dh={dh} Ktot={N + R_ + P} {fmt}: rel-L2 {err:.3e} (bar {TAP_BARS[fmt]:.1e})")
    assert err < TAP_BARS[fmt], f"{fmt}: {err:.3e}"
    assert np.array_equal(run(), got), "two runs differ"


def test_text_mass_all_keys_masked_and_other_streams(keng):
    """A row whose keys are ALL masked gives exactly 0 (never NaN); and the bits do not depend on what other streams are doing."""
    B, N, H, dh, P = 2, 9, 8, 64, 5
    qkvg = _rand(B, N, 4 * H * dh, seed=30)
    w = torch.ones(H, dh)
    rope = torch.zeros(N, dh)
    kt, vt = _rand(B, H, P, dh, seed=31), _rand(B, H, P, dh, seed=32)
    ms = torch.ones(B, N, dtype=torch.bool); ms[1] = False
    mt = torch.ones(B, P, dtype=torch.bool); mt[1] = False
    for fmt in ("bf16x3", "f16"):
        got = keng.test_attn_text_mass(qkvg, w, w, 1e-5, rope, dh, H, dh, None, None, kt, vt, ms, None, mt, fmt=fmt).cpu()
        assert torch.isfinite(got).all() and float(got[1].abs().max()) == 0.0 and float(got[0].min()) > 0
    args = _attn_inputs(16, 75, 8, 120, 64, 15, 30, 20, 18)
    qkvg, qw, kw, rope, kr, vr, kt, vt, ms, mr, mt = args
    call = lambda: keng.test_attn_text_mass(qkvg, qw, kw, 1e-6, rope, 64, 8, 120, kr, vr, kt, vt, ms, mr, mt, fmt="f16")
    alone = call().cpu()
    side = torch.cuda.Stream(keng.device)
    a, b = torch.randn(2048, 2048, device=keng.device), torch.randn(2048, 2048, device=keng.device)
    with torch.cuda.stream(side):
        for _ in range(20):
            a = (a @ b).tanh()
    busy = call().cpu()
    torch.cuda.synchronize()
    assert torch.equal(alone, busy)


# ---- a planted alignment: tap + path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f16", "bf16x3"])
def test_planted_alignment_is_recovered(keng, fmt):
    """Queries and text keys planted in the unrotated dims 64..119 (norm weights ones): frame n and text key pi(n) share a direction,
    pi monotone.  argmax_p mass[n] == pi(n) for every frame, and align_path returns exactly the planted spans — also behind a prefix."""
    H, dh, rot, N, P = 8, 120, 64, 40, 15
    ns, p0s = [40, 33], [0, 3]
    B = len(ns)
    D = H * dh
    g = torch.Generator().manual_seed(3)
    pis = [[p0s[b] + (n * (P - p0s[b])) // ns[b] for n in range(ns[b])] for b in range(B)]
    qkvg = torch.zeros(B, N, 4, H, dh)
    qkvg[:, :, 1, :, :rot] = torch.randn(B, N, H, rot, generator=g)        # self keys live in the rotated dims only: q . k_self = 0
    qkvg[:, :, 2:] = torch.randn(B, N, 2, H, dh, generator=g)
    kt = torch.zeros(B, H, P, dh)
    for p in range(P):
        kt[:, :, p, 64 + p] = 24.0                                          # logit of the planted key: sqrt(dh) e_p . 24 e_p / sqrt(dh) = 24
    for b in range(B):
        for n in range(ns[b]):
            qkvg[b, n, 0, :, 64 + pis[b][n]] = 1.0
    vt = torch.randn(B, H, P, dh, generator=g)
    ms = torch.arange(N)[None] < torch.tensor(ns)[:, None]
    ones = torch.ones(H, dh)
    inv = 1.0 / (1e4 ** (torch.arange(0, rot, 2).float() / rot))
    rope = (torch.arange(N).float()[:, None] * inv[None]).repeat_interleave(2, -1).contiguous()
    mass = keng.test_attn_text_mass(qkvg.reshape(B, N, 4 * D), ones, ones, 1e-6, rope, rot, H, dh, None, None, kt, vt, ms, None, None, fmt=fmt)
    spans, score = keng.align_path(mass, ns, p0s, [P] * B)
    mh, spans, score = mass.cpu().numpy(), spans.cpu().numpy(), score.cpu().numpy()
    for b in range(B):
        assert [int(v) for v in mh[b, :ns[b]].argmax(-1)] == pis[b], b
        assert float(mh[b, np.arange(ns[b]), pis[b]].min()) > 0.999
        want = R.spans_of_path([(n, pis[b][n]) for n in range(ns[b])], P)
        assert (want[:p0s[b]] == -1).all() and (want[p0s[b]:] >= 0).all()
        assert np.array_equal(spans[b], want), (b, spans[b].tolist(), want.tolist())
        assert 0 <= score[b] < 1e-3 * ns[b]
        ref_spans, ref_score, _ = R.dp_align(mh[b], ns[b], p0s[b], P)
        assert np.array_equal(spans[b], ref_spans) and score[b] == ref_score


# ---- the path kernel -----------------------------------------------------------------------------------------------------------------
PATH_CASES = {
    "75x30": (75, 30, [75, 40, 1, 75, 0, 75], [0, 5, 0, 29, 0, 7], [30, 30, 30, 30, 30, 7]),     # ragged, a one-token range, no frames, an empty token range
    "225x198": (225, 198, [225, 100, 225, 17], [0, 0, 150, 20], [198, 198, 198, 61]),
    "1x1": (1, 1, [1, 0], [0, 0], [1, 1]),
    "more tokens than frames": (12, 40, [12, 3], [0, 10], [40, 40]),
}


@pytest.mark.parametrize("case", list(PATH_CASES))
@pytest.mark.parametrize("peaky", [False, True])
def test_align_path_equals_the_restatement(keng, case, peaky):
    N, P, ns, p0s, p1s = PATH_CASES[case]
    B = len(ns)
    rng = np.random.default_rng(N * 1000 + P + peaky)
    mass = rng.random((B, N, P), dtype=np.float32)
    if peaky:   # softmax-like rows: most of the mass on a few columns, sums <= 1
        mass = mass ** 8
        mass /= np.maximum(mass.sum(-1, keepdims=True), 1e-9) * rng.uniform(1.0, 2.0, (B, N, 1)).astype(np.float32)
    run = lambda: keng.align_path(torch.from_numpy(mass).to(keng.device), ns, p0s, p1s)
    spans_d, score_d = run()
    spans, score = spans_d.cpu().numpy(), score_d.cpu().numpy()
    assert spans.shape == (B, P, 2) and spans.dtype == np.int32
    for b in range(B):
        ref_spans, ref_score, path = R.dp_align(mass[b], ns[b], p0s[b], p1s[b])
        assert np.array_equal(spans[b], ref_spans), (case, b)
        assert score[b] == ref_score, (case, b, score[b], ref_score)
        if path:
            assert np.array_equal(R.spans_of_path(path, P), spans[b])                       # the back-track itself
            f64 = R.path_score_f64(mass[b], path)
            assert abs(float(score[b]) - f64) <= (N + P) * 2.0 ** -24 * f64, (case, b, score[b], f64)
            assert spans[b, p0s[b], 0] == 0 and spans[b, p1s[b] - 1, 1] == ns[b] - 1
        else:
            assert (spans[b] == -1).all() and score[b] == 0
    s2, c2 = run()
    assert torch.equal(s2, spans_d) and torch.equal(c2, score_d)


def test_align_path_refuses_what_it_cannot_hold(keng):
    for N, P in ((226, 10), (10, 199)):
        with pytest.raises(ValueError, match="supported range"):
            keng.align_path(torch.zeros(1, N, P, device=keng.device), [1], [0], [1])
    import ctypes as C
    m = torch.zeros(1, 226, 10, device=keng.device)
    z = torch.zeros(1, dtype=torch.int32, device=keng.device)
    out = torch.zeros(1, 10, 2, dtype=torch.int32, device=keng.device)
    sc = torch.zeros(1, device=keng.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert keng.lib.smtts_align_path(keng.h, None, p(m), 1, 226, 10, p(z), p(z), p(z), p(out), p(sc)) == 1
    assert b"225" in keng.lib.smtts_last_error(keng.h)


# ---- the whole path: sample(align=...) -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deng(golden_seed):
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(golden_seed, parts=("dit",))
    e.finalize()
    return e


def _shape_inputs(shape):
    if shape == "small":
        g = golden("case_small.npz")
        ref, ref_len, ids = torch.from_numpy(g["ref"]), torch.from_numpy(g["ref_len"]), torch.from_numpy(g["ids"])
        pm, mask = torch.from_numpy(g["ph_mask"]), torch.from_numpy(g["mask"])
        noise = torch.randn(4, *g["x_t"].shape, generator=torch.Generator().manual_seed(2))
        return ref, ref_len, ids, pm, mask, noise
    gen = torch.Generator().manual_seed(0)                  # the bench shape: 8 x 10 s, R = 15, P = 30 (tests/test_dit_gpu.py)
    B, N, R_, P = 8, 75, 15, 30
    ref = torch.randn(B, R_, 64, generator=gen)
    ids = torch.arange(1, P + 1)[None].repeat(B, 1)
    noise = torch.randn(4, B, N, 64, generator=gen)
    return ref, torch.full((B,), R_), ids, torch.ones(B, P, dtype=torch.bool), torch.ones(B, N, dtype=torch.bool), noise


_ORACLE = {}


def _oracle_mass(dit_weights, shape, sel=None):
    key = (shape, sel)
    if key not in _ORACLE:
        ref, ref_len, ids, pm, mask, noise = _shape_inputs(shape)
        kw = {} if sel is None else dict(steps=sel.steps, layers=sel.layers, heads=sel.heads)
        with torch.no_grad():
            oc = O.encode_conditions(dit_weights, ref, ref_len, ids, pm)
            _ORACLE[key] = R.sampler_text_mass(dit_weights, oc, pm, mask, noise, 4, **kw)
    return _ORACLE[key]


@pytest.mark.parametrize("shape", ["small", "bench"])
@pytest.mark.parametrize("preset", ["bf16x3", "f16"])
def test_sample_align_latents_bit_identical_and_mass_vs_oracle(deng, dit_weights, shape, preset):
    ref, ref_len, ids, pm, mask, noise = _shape_inputs(shape)
    deng.set_precision(preset)
    try:
        cache = deng.cond_encode(ref, ref_len, ids, pm)
        plain = deng.sample(cache, mask, num_steps=4, noise=noise)
        x, mass = deng.sample(cache, mask, num_steps=4, noise=noise, align=True)
        x2, mass2 = deng.sample(cache, mask, num_steps=4, noise=noise, align=Alignment())
        again = deng.sample(cache, mask, num_steps=4, noise=noise)
    finally:
        deng.set_precision("bf16x3")
    assert torch.equal(x, plain) and torch.equal(x2, plain) and torch.equal(again, plain), "the tap moved the latents"
    assert torch.equal(mass, mass2)
    ox, om = _oracle_mass(dit_weights, shape)
    mh = mass.cpu().numpy()
    assert not mh[~mask.numpy()].any() and not mh.transpose(0, 2, 1)[~pm.numpy()].any()
    assert float(mh.sum(-1).max()) <= 1.0 + 1e-6
    err, lat = rel_l2(mh, om.numpy()), rel_l2(x.cpu().numpy(), ox.numpy())
    print(f"\n[sample align] {shape} {preset}: mass rel-L2 vs oracle {err:.3e} (bar {MASS_BARS[preset]:.2e}); latents {lat:.3e}")
    assert err < MASS_BARS[preset], f"{shape} {preset}: {err:.3e}"


def test_sample_align_selection_cfg_and_the_switched_off_image_path(deng, dit_weights):
    ref, ref_len, ids, pm, mask, noise = _shape_inputs("small")
    cache = deng.cond_encode(ref, ref_len, ids, pm)
    plain = deng.sample(cache, mask, num_steps=4, noise=noise)
    sel = Alignment(layers=(0, 5, 11), heads=(1, 6), steps=(0, -1))
    x, mass = deng.sample(cache, mask, num_steps=4, noise=noise, align=sel)
    assert torch.equal(x, plain)
    _, om = _oracle_mass(dit_weights, "small", sel)
    err = rel_l2(mass.cpu().numpy(), om.numpy())
    print(f"\n[sample align] small bf16x3, layers (0, 5, 11) x heads (1, 6) x steps (0, -1): mass rel-L2 vs oracle {err:.3e}")
    assert err < MASS_BARS["bf16x3"]
    one = deng.sample(cache, mask, num_steps=4, noise=noise, align=Alignment(layers=(3,), heads=(2,)))[1]
    assert not torch.equal(one, mass) and float(one.sum(-1).max()) <= 1.0 + 1e-6
    # CFG: 3B-row caches, only the B conditional rows are tapped; at step 0 x_t does not depend on the guidance, so the conditional
    # rows see the arithmetic of the plain run up to the batch shape's GEMM tiling
    B = ref.shape[0]
    ref3, len3, ids3, pm3 = O.cfg_conditions(ref, ref_len, ids, pm)
    cache3 = deng.cond_encode(ref3, len3, ids3, pm3)
    first = Alignment(steps=(0,))
    xc = deng.sample(cache3, mask, num_steps=4, mode="ode", cfg=True, noise=noise[0])
    xa, mc = deng.sample(cache3, mask, num_steps=4, mode="ode", cfg=True, noise=noise[0], align=first)
    assert torch.equal(xa, xc) and tuple(mc.shape) == (B, mask.shape[1], ids.shape[1])
    m1 = deng.sample(cache, mask, num_steps=4, mode="ode", noise=noise[0], align=first)[1]
    e = rel_l2(mc.cpu().numpy(), m1.cpu().numpy())
    print(f"[sample align] cfg rows vs plain rows at step 0: {e:.3e}")
    assert e < 2 * MASS_BARS["bf16x3"]      # both sides lie within the bar of the same oracle values
    # the lab switch turns the image path off: a tap request is an error, never a buffer of zeros; plain sampling still works
    deng._ck(deng.lib.smtts_test_set_attention_mfma(deng.h, 0), "set")
    try:
        with pytest.raises(RuntimeError, match="image path"):
            deng.sample(cache, mask, num_steps=4, noise=noise, align=True)
    finally:
        deng._ck(deng.lib.smtts_test_set_attention_mfma(deng.h, 1), "set")
    assert torch.equal(deng.sample(cache, mask, num_steps=4, noise=noise), plain)


# ---- public results --------------------------------------------------------------------------------------------------------------------
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


def _sentence(rng, n_words):
    """token ids of n_words random words with spaces, a comma and a full stop"""
    from smalltts_amd.phonemes import LATIN, p2idx
    out = []
    for i in range(n_words):
        out += [p2idx[LATIN[int(c)]] for c in rng.integers(0, len(LATIN), size=int(rng.integers(1, 6)))]
        out += [p2idx[","]] if i == n_words // 2 else []
        out += [p2idx[" "]]
    return out[:-1] + [p2idx["."]]


SHARP = dict(rel_db=3, min_run=1, floor_dbfs=-200)


def test_synthesize_batch_align_words_equal_the_restatement_on_the_returned_mass(tts, voice):
    rng = np.random.default_rng(5)
    toks = [_sentence(rng, 3), _sentence(rng, 6), [1, 2] + _sentence(rng, 4)]
    pre = [0, 0, 2]
    durs = [1.0, 2.2, 1.5]
    kw = dict(voices=[voice] * 3, seeds=[5, 6, 7])
    plain, plat = tts.synthesize_batch(None, toks, durs, return_latents=True, **kw)
    outs, lat, words, raw = tts.synthesize_batch(None, toks, durs, return_latents=True, align=True, prefix_lens=pre, return_alignment=True, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(outs, plain)) and all(np.array_equal(a, b) for a, b in zip(lat, plat))
    for b in range(3):
        mass, spans = raw[b]
        n = max(1, int(durs[b] * 7.5))
        assert mass.shape == (n, len(toks[b])) and spans.shape == (len(toks[b]), 2)
        ref_spans, _, _ = R.dp_align(mass, n, pre[b], len(toks[b]))
        assert np.array_equal(spans, ref_spans), b
        groups = token_groups(toks[b][pre[b]:])
        assert words[b] == word_times(groups, ref_spans, n, token0=pre[b]) and len(words[b]) == len(groups) > 2
        assert [w[0] for w in words[b]] == list(range(len(groups))) and [w[1] for w in words[b]] == [g[0] for g in groups]
        assert all(0 <= s <= e <= HOP_SIZE * n and s % HOP_SIZE == 0 for _, _, s, e in words[b])
        assert words[b][0][2] == 0 and words[b][-1][3] == HOP_SIZE * n
        assert [w[2] for w in words[b]] == sorted(w[2] for w in words[b])
    # with trim: the same spans, intersected with the speech window and counted from its start
    ep = Endpointing(**SHARP)
    cut, cwords = tts.synthesize_batch(None, toks, durs, trim=ep, align=True, prefix_lens=pre, **kw)
    ref_cut = tts.synthesize_batch(None, toks, durs, trim=ep, **kw)
    for b in range(3):
        assert np.array_equal(cut[b], ref_cut[b])
        nw = cut[b].shape[1]
        assert all(0 <= s <= e <= nw for _, _, s, e in cwords[b]) and len(cwords[b]) == len(words[b])
        d = [(w[2] - c[2], w[3] - c[3]) for w, c in zip(words[b], cwords[b]) if 0 < c[2] and c[3] < nw]
        assert len(set(d)) <= 1 and all(x == y for x, y in d)        # inside the window: one common shift, the window's start
    with pytest.raises(ValueError):
        tts.synthesize_batch(None, [list(range(1, 198)) + [1, 2]], [1.0], voices=[voice], align=True)       # 199 tokens
    with pytest.raises(ValueError):
        tts.synthesize_batch(None, toks, durs, prefix_lens=pre, **kw)
    with pytest.raises(TypeError):
        tts.synthesize_batch(None, toks, durs, align="yes", **kw)


def _long_kw():
    rng = np.random.default_rng(12)
    durs = [1.0, 2.2, 1.5, 0.7, 3.0, 1.2, 2.0, 0.5, 1.8, 2.6, 0.9]
    toks = [_sentence(rng, int(rng.integers(2, 6))) for _ in durs]
    return dict(token_lists=toks, durations=durs, seed=3, max_batch=4, in_flight=3), [max(1, int(d * 7.5)) for d in durs], toks


@pytest.mark.parametrize("trim", [False, True])
@pytest.mark.parametrize("prefix", [(), (1, 2, 3)])
def test_synthesize_long_words(tts, voice, trim, prefix):
    kw, ns, toks = _long_kw()
    ep = Endpointing(**SHARP) if trim else None
    extra = dict(prefix_tokens=list(prefix)) if prefix else {}
    base, bsegs = tts.synthesize_long(voice, trim=ep, return_segments=True, **extra, **kw)
    out, segs, words = tts.synthesize_long(voice, trim=ep, return_segments=True, return_words=True, **extra, **kw)
    only = tts.synthesize_long(voice, trim=ep, return_words=True, **extra, **kw)
    assert np.array_equal(out, base) and segs == bsegs and np.array_equal(only[0], out) and only[1] == words
    counts = [len(token_groups(t)) for t in toks]
    assert len(words) == sum(counts) and [w[0] for w in words] == list(range(len(words)))
    starts = [w[2] for w in words]
    assert starts == sorted(starts) and all(w[2] <= w[3] for w in words), "times must not go backwards through the text"
    # every word inside its piece's segment (with trim: the speech window as placed in the joined waveform)
    k = 0
    for i, c in enumerate(counts):
        off, n = segs[i][0], segs[i][1]
        assert all(off <= s <= e <= off + n for _, _, s, e in words[k:k + c]), i
        k += c
    # ... and equal to a piece-by-piece composition: the same pieces as batches of their own, mapped by hand
    seeds = [piece_seed(3, i) for i in range(len(toks))]
    want = []
    for g0 in range(0, len(toks), 4):
        g = list(range(g0, min(g0 + 4, len(toks))))
        _, raw_words, raw = tts.synthesize_batch(None, [list(prefix) + toks[i] for i in g], None, frames=[ns[i] for i in g], voices=[voice] * len(g),
                                                 seeds=[seeds[i] for i in g], align=True, prefix_lens=[len(prefix)] * len(g),
                                                 return_alignment=True)
        for r, i in enumerate(g):
            win = (segs[i][2], segs[i][1]) if trim else None
            want += word_times(token_groups(toks[i]), raw[r][1], ns[i], token0=len(prefix), window=win, offset=segs[i][0], index0=len(want))
    assert words == want
    if trim:
        print(f"\n[long words] trimmed: {sum(s[1] for s in segs)} of {sum(HOP_SIZE * n for n in ns)} samples kept, {len(words)} groups")
    with pytest.raises(ValueError):
        tts.synthesize_long(voice, align=Alignment(), **kw)


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


def test_server_align_round_trip(eng, tts):
    """align=1 answers the same audio bytes plus x-smtts-words, the spans the API gives for the same reference, tokens and noise;
    without the parameter (or align=0) the response is what it was: same bytes, no new header."""
    from http.server import ThreadingHTTPServer
    from smalltts_amd.api import Encoder
    enc = Encoder(engine=eng)
    batcher = S.Batcher(tts, enc, max_batch=8, window_ms=1.0, in_flight=2, num_steps=4)
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), S.make_handler(batcher, tokenizer="chars"))
    httpd.daemon_threads = True
    threading.Thread(target=httpd.serve_forever, kwargs={"poll_interval": 0.02}, daemon=True).start()
    port = httpd.server_address[1]
    t = np.arange(int(0.7 * 24000)) / 24000.0
    wav = S.encode_wav((0.4 * np.sin(2 * np.pi * 260 * t)).astype(np.float32), 24000)
    toks = _sentence(np.random.default_rng(9), 5)
    tok_s = ",".join(str(v) for v in toks)
    try:
        st0, h0, plain = _post(port, wav, tok_s, "duration=1.3&seed=77")
        st1, h1, off = _post(port, wav, tok_s, "duration=1.3&seed=77&align=0")
        st2, h2, on = _post(port, wav, tok_s, "duration=1.3&seed=77&align=1")
        st3, h3, cut = _post(port, wav, tok_s, "duration=1.3&seed=77&align=1&trim=1")
        st4, _, msg = _post(port, wav, tok_s, "duration=1.3&seed=77&align=2")
        st5, _, msg5 = _post(port, wav, tok_s, "duration=31&seed=77&align=1")
    finally:
        httpd.shutdown()
        httpd.server_close()
        batcher.close()
    assert st0 == st1 == st2 == st3 == 200 and st4 == st5 == 400 and b"`align`" in msg and b"`align`" in msg5
    assert plain == off == on and "x-smtts-words" not in h0 and "x-smtts-words" not in h1
    assert sorted(h0) == sorted(h1) and {k: v for k, v in h0.items() if k != "date"} == {k: v for k, v in h1.items() if k != "date"}
    got = json.loads(h2["x-smtts-words"])
    # the API on the same inputs: the server's reference latents, its per-request noise streams (seed 77), its frame count
    y, sr = S.decode_wav_bytes(wav)
    n = S.frames_for(1.3)
    lat = enc.encode_reference(torch.from_numpy(np.ascontiguousarray(y[: len(y) // HOP_SIZE * HOP_SIZE]))[None, None])[0].numpy()
    noise = torch.stack([eng.randn(n * 64, 77, s_).view(1, n, 64) for s_ in range(4)])
    prev = eng.set_tuning("throughput")                      # the server's tuning (the two differ by fp32 summation order)
    try:
        outs, words = tts.synthesize_batch([lat], [toks], None, frames=[n], noise=noise, align=True)
    finally:
        eng.set_tuning(prev)
    assert got == [[w[2], w[3]] for w in words[0]] and len(got) == len(token_groups(toks)) > 5
    assert outs[0].shape == (1, HOP_SIZE * n) and len(plain) == 44 + 2 * HOP_SIZE * n
    s, nw = int(h3["x-smtts-start"]), int(h3["x-smtts-samples"])
    cw = json.loads(h3["x-smtts-words"])
    assert cw == [[min(max(a - s, 0), nw), min(max(b - s, 0), nw)] for a, b in got] and len(cut) == 44 + 2 * nw
