"""GPU: the LN-fold (gemm.hpp LnFoldIn) one step at a time against an fp64 reference.

smtts_test_ln_fold runs one producer -> consumer step of the shipped chain: the gated residual of x with the EpiResidLN epilogue (residual,
operand image, per-32-column partials), the fold tables of fold_vectors_kernel, and the folded SwiGLU consumer — or, with fold=False,
the norm-launch path of the same step (plain residual, ln_modulate / rmsnorm, plain SwiGLU).  Both are held to

    x += mask gate (A Wp^T + bp);   y = LN(x) (1 + scale) + shift   (or RMSNorm(x) scale);   h = silu(y W1^T + b1) (y W3^T + b3)

in fp64.  The operands A, Wp, W1, W3 are rounded to the preset's 16-bit format first, so what is left of the error is the arithmetic of
the two paths: the normalisation, the operand image of y (norm path) or of x (1 + scale) (fold) and the 16-bit hidden image both write.
The fold must stay within 1.25x of the norm path's error at every row offset: a LayerNorm rewritten as E[x^2] - mu^2 on the raw row
loses the rows whose mean is large against their spread unless the producer takes a per-row constant out first."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PRECISIONS = ("f16", "bf16x3", "bf16")
ABS = {"bf16x3": 5e-5, "f16": 1.5e-3, "bf16": 1.2e-2}      # rel L2 of the hidden vs fp64 (norm path and fold alike)
FLOOR = {"bf16x3": 2e-6, "f16": 2e-5, "bf16": 2e-4}        # added to 1.25 x the norm path's error
X_TOL = 3e-5                                                 # residual update vs fp64 (exact operands: fp32 accumulation only)
K, F = 960, 256


def _round(t, precision):
    return {"f16": lambda a: a.half().float(), "bf16": lambda a: a.bfloat16().float(), "bf16x3": lambda a: a}[precision](t)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    return HipEngine(0)


def _case(M, D, precision, seed, offset=0.0, masked=0.2):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    sigma = 0.5 + 1.5 * torch.rand(M, 1, generator=g)
    sign = torch.where(torch.rand(M, 1, generator=g) < 0.5, -1.0, 1.0)
    x = sign * offset * sigma + sigma * r(M, D)                     # per-row, mixed-sign offsets |c| / sigma = offset
    c = dict(x=x, A=_round(r(M, K), precision), Wp=_round(r(D, K) / K ** 0.5, precision), bp=0.1 * r(D),
             gate=0.5 * r(D), scale=0.3 * r(D), shift=0.3 * r(D),
             W1=_round(r(F, D) / D ** 0.5, precision), W3=_round(r(F, D) / D ** 0.5, precision), b1=0.1 * r(F), b3=0.1 * r(F))
    c["row_mask"] = None if masked is None else (torch.rand(M, generator=g) >= masked)
    return c


def _reference(c, rms, eps=1e-6):
    d = {k: (v.double() if v is not None and v.dtype != torch.bool else v) for k, v in c.items()}
    upd = d["gate"] * (d["A"] @ d["Wp"].T + d["bp"])
    if d["row_mask"] is not None:
        upd = upd * d["row_mask"].double()[:, None]
    x = d["x"] + upd
    if rms:
        y = x / torch.sqrt((x * x).mean(1, keepdim=True) + eps) * d["scale"]
    else:
        mu = x.mean(1, keepdim=True)
        var = ((x - mu) ** 2).mean(1, keepdim=True)
        y = (x - mu) / torch.sqrt(var + eps) * (1 + d["scale"]) + d["shift"]
    a, b = y @ d["W1"].T + d["b1"], y @ d["W3"].T + d["b3"]
    return x, a * torch.sigmoid(a) * b


def _run(eng, c, rms, fold, precision, return_shift=False):
    out = eng.test_ln_fold(c["x"], c["A"], c["Wp"], c["scale"], c["W1"], c["W3"], shift=None if rms else c["shift"], bp=c["bp"],
                           gate=c["gate"], row_mask=c["row_mask"], b1=c["b1"], b3=c["b3"], rms=rms, fold=fold, precision=precision,
                           return_shift=return_shift)
    return tuple(t.cpu() for t in out)


def _check_shift(cs, x_ref, rms):
    """The row shift the consumer leaves for the next producer: the mean of the UPDATED row (LayerNorm; RMSNorm has none).  The chain
    relies on it: a stale or reset shift brings back the cancellation of the unshifted fold on the next producer."""
    if rms:
        assert torch.count_nonzero(cs) == 0
        return
    mu, sd = x_ref.mean(1), x_ref.std(1)
    err = ((cs.double() - mu).abs() / (mu.abs() + sd)).max().item()
    assert err < 1e-5, f"row shift vs mean of the updated row: worst {err:.3e} (relative to |mean| + std)"


def _check_x(c, x, x_ref):
    live = torch.ones(x.shape[0], dtype=torch.bool) if c["row_mask"] is None else c["row_mask"]
    if (~live).any():
        assert torch.equal(x[~live], c["x"][~live]), "masked rows must keep x bit for bit"
    if live.any():
        e = _rel(x[live] - c["x"][live], x_ref[live] - c["x"][live].double())
        assert e < X_TOL, f"residual update rel L2 {e:.3e}"


@pytest.mark.parametrize("M", [1, 37, 64, 600, 1024, 1500])
@pytest.mark.parametrize("rms,D", [(0, 960), (1, 960), (1, 512)])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ln_fold_step_matches_fp64_and_the_norm_launches(eng, precision, rms, D, M):
    """Plain parity on rows of mean ~ 0, a ragged row mask (none at M = 64)."""
    c = _case(M, D, precision, seed=M * 7 + D + rms, masked=None if M == 64 else 0.2)
    x_ref, h_ref = _reference(c, rms)
    x_n, h_n = _run(eng, c, rms, False, precision)
    x_f, h_f, cs = _run(eng, c, rms, True, precision, return_shift=True)
    _check_x(c, x_n, x_ref)
    _check_x(c, x_f, x_ref)
    _check_shift(cs, x_ref, rms)
    e_norm, e_fold = _rel(h_n, h_ref), _rel(h_f, h_ref)
    print(f"\n[ln-fold step {precision} rms={rms} D={D} M={M}] hidden vs fp64: norm launches {e_norm:.3e}, fold {e_fold:.3e}")
    assert e_norm < ABS[precision] and e_fold < ABS[precision]
    assert e_fold <= 1.25 * e_norm + FLOOR[precision]


@pytest.mark.parametrize("offset", [0, 1, 3, 10, 30, 100])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ln_fold_on_rows_with_a_large_mean(eng, precision, offset):
    """x_in = c_m + sigma_m z with per-row, mixed-sign c_m, |c_m| / sigma_m = offset: LayerNorm does not see c_m, neither may the fold."""
    M, D = 600, 960
    c = _case(M, D, precision, seed=1000 + offset, offset=float(offset))
    x_ref, h_ref = _reference(c, 0)
    x_n, h_n = _run(eng, c, 0, False, precision)
    x_f, h_f, cs = _run(eng, c, 0, True, precision, return_shift=True)
    _check_x(c, x_f, x_ref)
    _check_shift(cs, x_ref, 0)
    e_norm, e_fold = _rel(h_n, h_ref), _rel(h_f, h_ref)
    print(f"\n[ln-fold offset {precision} |c|/sigma={offset}] hidden vs fp64: norm launches {e_norm:.3e}, fold {e_fold:.3e}")
    assert e_norm < ABS[precision]
    assert e_fold <= 1.25 * e_norm + FLOOR[precision], f"|c|/sigma = {offset}: fold {e_fold:.3e} vs norm launches {e_norm:.3e}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ln_fold_on_constant_and_nearly_constant_rows(eng, precision):
    """Masked rows keep x and still feed the image and the statistics: rows that are constant (sigma = 0: LN(x) = 0, h depends on
    W shift + b only) or nearly so (sigma = 1e-3 |c|) go through both paths unchanged by the residual."""
    M, D = 96, 960
    c = _case(M, D, precision, seed=77)
    g = torch.Generator().manual_seed(78)
    consts = torch.tensor([0.5, 10.0, -3.0, 0.1, 100.0, -0.7])
    for i in range(M // 2):
        cm = consts[i % len(consts)]
        c["x"][i] = cm if i % 2 == 0 else cm + 1e-3 * abs(cm) * torch.randn(D, generator=g)
    c["row_mask"] = torch.arange(M) >= M // 2           # the constant rows are masked: x stays what it is
    x_ref, h_ref = _reference(c, 0)
    x_n, h_n = _run(eng, c, 0, False, precision)
    x_f, h_f = _run(eng, c, 0, True, precision)
    _check_x(c, x_f, x_ref)
    rows = {"sigma = 0": torch.arange(0, M // 2, 2), "sigma = 1e-3 |c|": torch.arange(1, M // 2, 2), "live": torch.arange(M // 2, M)}
    for name, sel in rows.items():
        e_norm, e_fold = _rel(h_n[sel], h_ref[sel]), _rel(h_f[sel], h_ref[sel])
        print(f"\n[ln-fold {precision} {name} rows] hidden vs fp64: norm launches {e_norm:.3e}, fold {e_fold:.3e}")
        # ln_modulate's fp32 mean of values ~ |c| is off by ~2^-24 |c| sqrt(D / 64): up to ~1e-4 of the spread at |c| / sigma = 1000
        # (measured 6.4e-5 at bf16x3); the fold takes that same mean as its row shift and sums x - c, which is exact there
        slack = 2e-4 if name.startswith("sigma = 1e-3") else 0.0
        assert e_norm < ABS[precision] + slack, f"{name}: norm launches {e_norm:.3e}"
        assert e_fold < ABS[precision], f"{name}: fold {e_fold:.3e}"
        assert e_fold <= 1.25 * e_norm + FLOOR[precision], f"{name}: fold {e_fold:.3e} vs norm launches {e_norm:.3e}"


@pytest.mark.parametrize("D", [480, 800])
def test_ln_fold_refuses_an_odd_number_of_partial_groups(eng, D):
    """The consumer reduces a row's D / 32 partials in pairs: an odd count would drop the last group, so the engine refuses to fold
    there (the encoders' fold condition is D % 64 == 0 for the same reason)."""
    c = _case(8, D, "f16", seed=D)
    with pytest.raises(RuntimeError, match="even number of 32-column partial groups"):
        _run(eng, c, 1, True, "f16")


def test_ln_fold_layernorm_tables_need_the_dit_width(eng):
    c = _case(8, 512, "f16", seed=3)
    with pytest.raises(RuntimeError, match="K = 960"):
        _run(eng, c, 0, True, "f16")


@pytest.mark.parametrize("rms", [0, 1])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ln_fold_step_is_bit_repeatable(eng, precision, rms):
    c = _case(600, 960, precision, seed=11, offset=10.0)
    a, b = _run(eng, c, rms, True, precision), _run(eng, c, rms, True, precision)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("case", ["small", "cfgrows", "bench1"])
def test_encoder_rmsnorm_fold_vs_norm_launches_and_reference_golden(golden_seed, case):
    """The condition encoders fold their RMSNorms (latency tuning, the default): per-layer K / V with the fold on and off, each against
    the reference golden at the split-bf16 tolerance of tests/test_dit_gpu.py, and against each other."""
    from smalltts_amd.engine import HipEngine
    from tests.conftest import golden, rel_l2
    TOL = 1e-4
    g = golden(f"case_{case}.npz")
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(golden_seed, parts=("dit",))
    e.finalize()
    assert e.set_tuning("latency") == "latency"
    caches = {}
    try:
        for on in (True, False):
            e.set_ln_fold(on)
            caches[on] = {k: v.cpu().numpy() for k, v in e.cond_encode(g["ref"], g["ref_len"], g["ids"], g["ph_mask"], debug=True).items()}
    finally:
        e.set_ln_fold(True)
    worst = 0.0
    for key in [k for k in g if k.startswith("L")]:
        li, name = key[1:].split("_", 1)
        km = g["ref_mask"] if name.endswith("ref") else g["ph_mask"]
        sel = np.broadcast_to(km[:, None, :, None], caches[True][name][int(li)].shape)
        got = {on: caches[on][name][int(li)][sel] for on in (True, False)}
        for on in (True, False):
            err = rel_l2(got[on], g[key][sel])
            assert err < TOL, f"{key} (fold {'on' if on else 'off'}): {err:.3e}"
        d = rel_l2(got[True], got[False])
        worst = max(worst, d)
        assert d < TOL, f"{key}: fold on vs off {d:.3e}"
    print(f"\n[encoder fold, {case}] per-layer K / V, fold on vs off: worst rel L2 {worst:.3e}")


def _sampler_inputs(B=4, N=40, R=10, P=12, seed=21):
    g = torch.Generator().manual_seed(seed)
    ref = torch.randn(B, R, 64, generator=g)
    ids = torch.randint(1, 198, (B, P), generator=g)
    pm = torch.ones(B, P, dtype=torch.bool)
    mask = torch.arange(N)[None] < torch.tensor([40, 31, 40, 17])[:, None]
    noise = torch.randn(4, B, N, 64, generator=g)
    return ref, torch.full((B,), R), ids, pm, mask, noise


@pytest.mark.parametrize("k", [0, 10, 30])
def test_dc_offset_residual_rows_through_the_sampler(k):
    """Seeded DiT weights with a constant added to the input embedding's output bias: every residual row's mean moves by k x the row std of
    the block-0 input, through all 12 blocks and every fold producer / consumer of the fused sampler (latency tuning: the fold is on),
    including the row shift each consumer advances.  At the shipped precision and at split-bf16, the fold and the norm launches are
    each held to the oracle at the suite's bounds, and the fold to the norm launches' error; no fp16 producer may clamp (the test is
    about conditioning, not range)."""
    from oracle import dit_oracle as O
    from smalltts_amd.engine import HipEngine
    from smalltts_amd.weights import dit_param_specs, synth_state_dict
    from tests.conftest import rel_l2
    bound = {"f16": 3e-4, "bf16x3": 1e-4}   # tests/test_precision_gpu.py TOL_F16, tests/test_dit_gpu.py TOL
    ref, ref_len, ids, pm, mask, noise = _sampler_inputs()
    sd = synth_state_dict(dit_param_specs(), 31)
    with torch.no_grad():
        std = O.input_embedding(O.to_torch(sd), noise[0], mask)[mask].std(-1).mean().item()
    # (on dit.input_embed.proj.bias the constant also feeds the conv pos-embed, whose grouped conv + Mish grows the row spread with
    # it: the block-0 rows then sit at mean / std ~ 3.5 for k = 10 and 30 alike.  On conv2's bias it arrives as a mean shift — Mish is
    # the identity for large arguments — and the rows sit at mean / std ~ k)
    sd["dit.input_embed.conv_pos_embed.conv2.bias"] = sd["dit.input_embed.conv_pos_embed.conv2.bias"] + np.float32(k * std)
    w = O.to_torch(sd)
    with torch.no_grad():
        h0 = O.input_embedding(w, noise[0], mask)[mask]
        ox = O.sample_dmd(w, O.encode_conditions(w, ref, ref_len, ids, pm), pm, mask, noise, 4).numpy()
    ratio = (h0.mean(-1).abs() / h0.std(-1)).mean().item()
    assert ratio > 0.5 * k, f"block-0 rows at mean / std {ratio:.1f}: the offset did not reach the residual stream"
    e = HipEngine(0)
    e.load_state_dict(sd)
    e.finalize()
    assert e.set_tuning("latency") == "latency"
    m = mask.numpy()
    print(f"\n[dc offset k={k}] block-0 input: row mean / row std {ratio:.1f}")
    try:
        for prec in ("f16", "bf16x3"):
            e.set_precision(prec)
            cache = e.cond_encode(ref, ref_len, ids, pm)
            e.saturations(reset=True)
            e.set_ln_fold(True)
            x_fold = e.sample(cache, mask, num_steps=4, noise=noise).cpu().numpy()
            e.set_ln_fold(False)
            x_norm = e.sample(cache, mask, num_steps=4, noise=noise).cpu().numpy()
            e.set_ln_fold(True)
            sat = e.saturations()
            e_fold, e_norm = rel_l2(x_fold[m], ox[m]), rel_l2(x_norm[m], ox[m])
            print(f"[dc offset k={k}, {prec}] latent vs oracle: fold {e_fold:.3e}, norm launches {e_norm:.3e}")
            assert not any(sat.values()), sat
            assert e_fold < bound[prec] and e_norm < bound[prec]
            assert e_fold < 1.25 * e_norm + 2e-5, f"{prec}: fold {e_fold:.3e} vs norm launches {e_norm:.3e}"
    finally:
        e.close()


def test_no_fold_tables_without_the_attention_epilogue(monkeypatch, golden_seed, dit_weights):
    """The fold needs the QKV GEMM's epilogue (EpiQKV) as its consumer: with SMTTS_ATTN_EPI=0 the sampler must not fold, must not
    build the fold tables (no fold_vectors launch), and still meet the oracle."""
    from oracle import dit_oracle as O
    from smalltts_amd.engine import HipEngine
    from tests.conftest import rel_l2
    monkeypatch.setenv("SMTTS_ATTN_EPI", "0")
    ref, ref_len, ids, pm, mask, noise = _sampler_inputs()
    with torch.no_grad():
        ox = O.sample_dmd(dit_weights, O.encode_conditions(dit_weights, ref, ref_len, ids, pm), pm, mask, noise, 4).numpy()
    e = HipEngine(0, "bf16x3")
    try:
        e.load_synthetic(golden_seed, parts=("dit",))
        e.finalize()
        assert e.set_tuning("latency") == "latency"
        cache = e.cond_encode(ref, ref_len, ids, pm)
        e.profile(True)
        x = e.sample(cache, mask, num_steps=4, noise=noise).cpu().numpy()
        torch.cuda.synchronize()
        names = [k["name"] for k in e.profile_report()]
        e.profile(False)
        assert names and not any("fold_vectors" in n for n in names), names
        m = mask.numpy()
        err = rel_l2(x[m], ox[m])
        print(f"\n[SMTTS_ATTN_EPI=0] latent vs oracle {err:.3e}")
        assert err < 1e-4
    finally:
        e.close()
