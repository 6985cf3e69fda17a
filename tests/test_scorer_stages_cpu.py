"""CPU: the per-stage references, bounds and weight families of the scorer stage tests hold what they promise, from the references
alone (tests/helpers/sv_stages.py, asr_stages.py, stage_bounds.py, scorer_families.py; the GPU side: tests/test_scorer_stages_gpu.py).

  * the family conditions (scorer_families.SV_CONDITIONS / ASR_CONDITIONS) on every randn case;
  * every stage helper composed in order is the whole restatement (embed_rows / logprobs_rows), in the layout of the device's taps;
  * the bound is sharp: a broken copy of a stage's reference, fed the same inputs, exceeds that stage's bound.  The copies: both
    operands of one product rounded to bfloat16 (every product of every stage), reflect replaced by edge repeat, the row constant
    omitted, the uniform std in place of the weighted one, one key dropped from the attention, the ninth conv tap dropped at frames
    t = 55 mod 56, the half-step 0.5 replaced by 1.  Inputs are the reference's own taps rounded to fp32 (what a device holds).

Sharpness, measured (worst |broken - reference| / bound; `pytest -s` prints every figure).  The bound counts n roundings for an n-term
sum whatever its order and sends an error through a following product by the absolute weights, so it stands two to four orders above
what fp32 really loses in the long sums (the device's own figures: tests/test_scorer_stages_gpu.py).  A bfloat16 operand (2^-9) still
exceeds it in every product of every stage.  ReLU and the sigmoid pass an error on by their Lipschitz constant over the interval the
error allows (stage_bounds.relu, sigmoid_lip): a unit that is dead beyond its own error passes nothing.  That is what makes the
squeeze-excite gate sharp (time mean, 768 -> 192, ReLU, 192 -> 768, sigmoid in one launch, nothing tapped inside): with the constants
1 and 1/4 everywhere a bfloat16 pair reached 0.75 (first product) and 0.62 (second) of its bound; now, under the shipped weights and
randn latents, 1.12 - 1.40 and 1.05 - 1.50 on every case, at gates between 0.002 and 0.999 (median ratio 0.2 - 0.3, 0.1 - 3 % of the
768 gates beyond 1); under the calibrated family 0.55 - 1.50.  Where a stage ends in ReLU + BatchNorm the worst ratio is now that
of a unit the bfloat16 operand revives (its bound is the rounding of the BatchNorm shift alone), hence the large figures.
Worst ratios, shipped weights / family: verifier blocks.0 1.4e7 / 1.5e5, tdnn1 8.4e8 / 1.4e5, res2net 1.2e9 / 1.4e5, tdnn2 3.2e9 /
1.3e5, mfa 4.4e8 / 4.1e4 (with ReLU's constant 1 everywhere they were 93 / 93, 20 / 14, 130 / 97, 21 / 13, 4.9 / 2.4: sharp either
way), gate 1.54 / 1.50 and 1.50 / 1.19 (over every case), se apply 1.0e5 /
1.2e5, stats 2.1e3 / 1.3e3, row constant (K = 4608) 1.11 / 0.99, attention 1.6e6 / 1.8, logits 63 / 81, pooling 4.0e3 / 6.3e3, fc
(K = 4608) 1.22 / 1.06; recogniser upsample 9.5e4, ffn1 2.8 / 2.8 (W1 / W2), qkv 171, scores 1.1e3, p v 505, proj 483, conv 5.0 /
4.8 / 5.6, ffn2 with the final LayerNorm 1.36 / 1.14, head 197.  The structural copies: edge repeat 6.9e10 (blocks.0) and 1.8e11
(res2net), no row constant 1.7e9 / 1.1e8, uniform std 5.5e4 / 1.3e7, dropped key 7.9e4 / 1.3e6, ninth tap 397, full step 1.1e3
(ffn1) and 392 (ffn2)."""
import pytest
import torch

from tests.helpers import asr_ref, asr_stages as AS, scorer_families as SF, sv_ref, sv_stages as SS
from tests.helpers.stage_bounds import ratio

torch.set_grad_enabled(False)
STAGES = {"sv": SS, "asr": AS}
MIN_N = {"sv": 6, "asr": 1}
SHARP_CASES = {"sv": [("randn", 2, 40, [40, 33]), ("randn", 1, 129, [129])], "asr": [("randn", 2, 29, [29, 16]), ("randn", 1, 65, [65])]}
SHARP_FAMILIES = {"sv": ("synth", "calibrated+peaked"), "asr": ("synth", "peaked")}
# stage kind (the slot name without its block / layer): the broken copies
MUTANTS = {
    "sv": {"blocks.0": ["bf16", "edge"], "tdnn1": ["bf16"], "res2net": ["bf16", "edge"], "tdnn2": ["bf16"], "gate": ["bf16:1", "bf16:2"],
           "out": ["bf16"], "mfa": ["bf16"], "stats": ["bf16"], "crow": ["bf16"], "att": ["bf16", "no_crow"], "logit": ["bf16"],
           "pooled": ["bf16", "uniform_std"], "emb": ["bf16"]},
    "asr": {"upsample": ["bf16"], "ffn1": ["bf16:1", "bf16:2", "full_step"], "qkv": ["bf16"], "attn": ["bf16:1", "bf16:2", "drop_key"],
            "proj": ["bf16"], "conv": ["bf16:1", "bf16:2", "bf16:3", "tap9"], "ffn2": ["bf16:1", "bf16:2", "full_step"], "logp": ["bf16"]},
}
PER_ROW = ("gate", "crow", "emb")      # stages of a few hundred elements a row: every case and family (the worst element decides)


def kind(name):
    return name if name == "blocks.0" else name.split(".")[-1]


_taps = {}


def ref_taps(net, fam, case):
    key = (net, fam, SF.case_id(case))
    if key not in _taps:
        x = SF.latents(case[0], case[1], case[2])
        _taps[key] = (x, STAGES[net].ref_taps(SF.model(net, fam), x, case[3]))
    return _taps[key]


# ---- families ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["calibrated", "calibrated+peaked"])
def test_verifier_families_put_every_stage_in_its_live_range(fam):
    m, C = SF.model("sv", fam), SF.SV_CONDITIONS
    ec = m.ecapa
    for case in [c for c in SF.SV_CASES if c[0] == "randn"] + [("randn", 1, 40, [40])]:
        x, taps = ref_taps("sv", fam, case)
        for b, n in enumerate(case[3]):
            if n < 6:
                continue
            mfa = taps["mfa"][b, :n]
            W = ec.asp.tdnn.conv.conv.weight[:, :2304, 0]
            sc, sh = SS._fold(ec.asp.tdnn.norm)
            arg = torch.relu(mfa @ W.T + ec.asp.tdnn.conv.conv.bias + taps["crow"][b]) * sc + sh
            gates = torch.stack([taps[f"blocks.{i}.gate"][b] for i in (1, 2, 3)])
            beyond = float((arg.abs() > 3).double().mean())
            const = int(((mfa.max(0).values - mfa.min(0).values) == 0).sum())
            peak = float(torch.softmax(taps["logit"][b, :n], 0).max(0).values.median())
            print(f"sv {fam} {SF.case_id(case)} row {b}: tanh arguments beyond 3: {beyond:.3f}, gates [{float(gates.min()):.3f}, "
                  f"{float(gates.max()):.3f}], constant MFA channels {const}, median largest pooling weight {peak:.3f}")
            assert beyond <= C["tanh_beyond_3"]
            assert C["gate_lo"] < float(gates.min()) and float(gates.max()) < C["gate_hi"]
            # (ReLU leaves a channel dead in all n frames with probability 2^-n whatever the statistics: 36 of 2304 at n = 6)
            assert const == 0 if n >= 32 else const <= 3 * 2304 * 2.0 ** -n, (n, const)
            if fam == "calibrated+peaked" and n == 40:
                assert peak >= C["peak_median"]
    # nothing but the BatchNorm statistics (and the scaled asp.conv.weight) differs from the shipped synthetic weights
    base, st = SF.state("sv", "synth"), SF.state("sv", fam)
    changed = {k for k in base if not torch.equal(base[k], st[k])}
    assert changed and all(k.endswith(("running_mean", "running_var")) or k == "ecapa.asp.conv.conv.weight" for k in changed)
    assert ("ecapa.asp.conv.conv.weight" in changed) == (fam == "calibrated+peaked")


def test_recogniser_peaked_family_has_peaked_attention_and_confident_frames():
    C = SF.ASR_CONDITIONS
    for case in [c for c in SF.ASR_CASES if c[0] == "randn"]:
        x, taps = ref_taps("asr", "peaked", case)
        for b, n in enumerate(case[3]):
            if n < 14:
                continue                                                   # (a row of 4 frames is peaked by counting)
            meds = [float(AS.attention_weights(taps[f"layers.{l}.qkv"][b, :4 * n]).max(-1).values.median()) for l in range(7)]
            conf = float((taps["logp"][b, :4 * n].exp().max(-1).values >= C["confident"]).double().mean())
            print(f"asr peaked {SF.case_id(case)} row {b}: attention medians {[round(v, 2) for v in meds]}, confident frames {conf:.2f}")
            assert sum(v >= C["attn_median"] for v in meds) >= C["attn_layers"]
            assert conf >= C["confident_frames"]


def test_recogniser_norms_family_spans_two_decades_with_both_signs():
    st = SF.state("asr", "norms")
    ln = [v for k, v in st.items() if v.dim() == 1 and (k.endswith("norm.weight") or k.endswith("sequential.0.weight"))]
    assert len(ln) == 7 * 5
    for w in ln:
        assert (w < 0).any() and (w > 0).any() and 0.1 <= float(w.abs().min()) and float(w.abs().max()) <= 10.0
        assert float(w.abs().max() / w.abs().min()) > 30.0
    var = torch.cat([v for k, v in st.items() if k.endswith("running_var")])
    assert 0.01 <= float(var.min()) < 0.02 and 0.5 < float(var.max()) <= 1.0


# ---- composition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,fam", [("sv", "synth"), ("sv", "calibrated+peaked"), ("asr", "synth"), ("asr", "peaked"), ("asr", "norms")])
def test_stage_helpers_composed_in_order_are_the_whole_restatement(net, fam):
    m = SF.model(net, fam)
    for case in SF.CASES[net][:3] + SF.CASES[net][5:]:
        x, taps = ref_taps(net, fam, case)
        whole = sv_ref.embed_rows(m, x, case[3]) if net == "sv" else asr_ref.logprobs_rows(m, x, case[3])
        last = taps["emb" if net == "sv" else "logp"]
        scale = float(whole.abs().max())
        assert float((last - whole).abs().max()) <= 1e-11 * max(scale, 1.0), (SF.case_id(case), float((last - whole).abs().max()), scale)
        for b, n in enumerate(case[3]):                                  # the layout: NaN exactly where the device writes nothing
            for name, t in taps.items():
                if t.dim() == 3 and name != "logp":
                    live = n * (4 if net == "asr" else 1) if n >= MIN_N[net] else 0
                    assert torch.isfinite(t[b, :live]).all() and torch.isnan(t[b, live:]).all(), (name, b)


# ---- sharpness --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,stage", [(net, k) for net in ("sv", "asr") for k in MUTANTS[net]])
def test_a_broken_stage_reference_exceeds_the_stages_bound(net, stage):
    M = STAGES[net]
    names = [n for n in M.NAMES if kind(n) == stage]
    dull = []
    for mut in MUTANTS[net][stage]:
        worst = {}
        for fam in (SF.SV_FAMILIES if stage in PER_ROW else SHARP_FAMILIES[net]):
            m = SF.model(net, fam)
            for case in (SF.CASES[net] if stage in PER_ROW else SHARP_CASES[net]):
                x, taps = ref_taps(net, fam, case)
                held = {k: v.float() for k, v in taps.items()}
                for b, n in enumerate(case[3]):
                    for name in names if n >= MIN_N[net] else []:
                        ref, bound = M.stages(m, held, x, n, b, only=[name])[name]
                        broken = M.stages(m, held, x, n, b, only=[name], mut=mut)[name][0]
                        worst[fam] = max(worst.get(fam, 0.0), ratio(broken, ref, bound))
        print(f"{net} {stage} {mut}: worst |broken - reference| / bound " + ", ".join(f"{f} {v:.3g}" for f, v in worst.items()))
        if not max(worst.values()) > 1.0:
            dull.append((mut, worst))
    assert not dull, (net, stage, dull)
