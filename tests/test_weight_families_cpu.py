"""CPU: what tests/test_weight_families_gpu.py rests on, shown on the fp64 reference alone (tests/helpers/weight_families.py,
oracle/dit_stages.py Rounding).

- the weight families are deterministic in (name, family, seed), change only the tensors they name and have the structure they claim;
- the rounding stand-in changes nothing while it is off;
- the amplification A = max(1, e_model / e0) of every case the GPU test bounds stays at or below 8 on EVERY row and utterance it
  compares, and the stand-in's operands stay at or below 65504 / 4 at every fp16 site (a clamp would change what is bounded);
- near-miss references (the slips the GPU cases are there to catch) miss the GPU test's allowance, BOUND x A + the fp32 floor, by at
  least 3x against the stand-in's own output, under the family that makes each of them count.

The families' constants are NOT the first ones tried: a common mode of 2 std(W) on every matrix, columns scaled by 8^u without a
renormalisation and norm weights of +- 8^u each broke the cap or the fp16 range on the stand-in (operands of 1e13, A in the
thousands), and so did modulation scales uniform over [-0.99, 4] (A up to 15 on the emitted image at f16).  As held here: common
mode 0.1 std(W); columns 8^u at unit mean square; norm weights +- 4^u; scales -0.99 + 4.99 v^16 (v uniform: most channels near
1 + scale = 0.01, one in sixteen above 2), shifts +- 3, gate pre-activations +- 5."""
import numpy as np
import pytest
import torch

from oracle import dit_stages as DS
from tests.helpers import weight_families as WF

NAMES = ["dit.transformer_blocks.0.attn_norm.linear.weight", "dit.transformer_blocks.0.attn_norm.linear.bias",
         "dit.norm_out.linear.bias", "dit.transformer_blocks.1.ff.w1.weight", "dit.transformer_blocks.1.ff.w1.bias",
         "dit.transformer_blocks.0.attn.q_norm.weight", "dit.transformer_blocks.11.attn.k_norm_cross.weight",
         "style_encoder.blocks.0.attention_norm.weight", "style_encoder.log_scale", "style_encoder.out_proj.weight",
         "phoneme_embedding.blocks.1.mlp.w2.weight", "dit.input_embed.conv_pos_embed.conv1.weight", "velocity.weight", "velocity.bias"]


@pytest.mark.parametrize("fam", WF.FAMILIES)
def test_families_are_deterministic_and_change_only_what_they_name(fam):
    sd = WF.base_sd()
    a, b, c = WF.family(sd, fam, 13), WF.family(sd, fam, 13), WF.family(sd, fam, 14)
    for k in NAMES:
        if WF.changes(fam, k, sd[k]):
            assert a[k].dtype == np.float32 and a[k].shape == sd[k].shape
            assert np.array_equal(a[k], b[k]), k
            if fam != "zero" and k != "style_encoder.log_scale":
                assert not np.array_equal(a[k], c[k]) and not np.array_equal(a[k], sd[k]), k
        else:
            assert a[k] is sd[k], k
    changed = set(a.changed())
    mats = {k for k, v in sd.items() if v.ndim == 2 and k.endswith(".weight") and "norm" not in k.rsplit(".", 2)[-2]}
    norms = {k for k in sd if k.endswith(("norm.weight", "norm_cross.weight"))}
    modlin = {k for k in sd if ".attn_norm.linear." in k or k.startswith("dit.norm_out.linear.")}
    want = {"zero": modlin, "common": mats, "colscale": mats, "heavy": mats, "norms": norms | {"style_encoder.log_scale"},
            "mod": {k for k in modlin if k.endswith(".bias")}}[fam]
    assert changed == want
    assert set(a.changed(NAMES)) == want & set(NAMES)


def test_families_have_the_structure_they_claim():
    sd = WF.base_sd()
    k = "dit.transformer_blocks.1.ff.w1.weight"
    w0 = sd[k].astype(np.float64)
    w = WF.family(sd, "common", 13)[k].astype(np.float64)
    assert np.allclose(w - w.mean(1, keepdims=True), w0 - w0.mean(1, keepdims=True), atol=1e-7)       # only the row means move
    assert 0.8 < (w.mean(1) - w0.mean(1)).std() / (WF.K["common"] * w0.std()) < 1.2
    r = WF.family(sd, "colscale", 13)[k].astype(np.float64) / w0
    assert np.allclose(r, r[:1], rtol=1e-5) and r[0].max() / r[0].min() > 40 and abs((r[0] ** 2).mean() - 1) < 1e-5
    h = WF.family(sd, "heavy", 13)[k].astype(np.float64)
    assert abs(h.std() / w0.std() - 1) < 1e-5 and np.abs(h).max() > 20 * h.std() > 0          # (uniform: max = 1.73 std)
    q = WF.family(sd, "norms", 13)["dit.transformer_blocks.0.attn.q_norm.weight"]
    assert 0.2 < (q < 0).mean() < 0.4 and np.abs(q).max() / np.abs(q).min() > 10 and np.abs(q).max() <= WF.K["normbase"]
    assert float(WF.family(sd, "norms", 13)["style_encoder.log_scale"]) == -0.5
    m = WF.family(sd, "mod", 13)["dit.transformer_blocks.0.attn_norm.linear.bias"].reshape(6, 960)
    for sh, sc, g in (m[0:3], m[3:6]):
        assert sc.min() < -0.95 and sc.min() >= -0.99 and 3.0 < sc.max() <= 4.0 and np.abs(sh).max() > 2.9 and np.abs(g).max() > 4.9
    z = WF.family(sd, "zero", 13)
    assert not z["dit.norm_out.linear.weight"].any() and not z["dit.transformer_blocks.5.attn_norm.linear.bias"].any()


def test_massive_input_and_stage_names():
    c, p = WF.case("blocks", 1, 0, 2, True), WF.case("blocks", 1, 0, 2, False)
    u = WF.MASSIVE_UTT
    other = [i for i in range(960) if i not in WF.MASSIVE_CH]
    assert torch.equal(c.x[:, :, other], p.x[:, :, other]) and torch.equal(c.x[:u], p.x[:u]) and torch.equal(c.x[u + 1:], p.x[u + 1:])
    ratio = c.x[u][:, list(WF.MASSIVE_CH)] / p.x[u].std(-1, keepdim=True)
    assert torch.allclose(ratio, torch.full_like(ratio, 300.0), rtol=1e-5)
    assert float((p.x[-1].mean(-1) / p.x[-1].std(-1)).abs().min()) > 50      # the utterance at mean 100 x its spread stays
    names = list(WF.base_sd())
    st = set(WF.stage_names(names))
    assert "dit.transformer_blocks.11.ff.w2.weight" in st and "dit.transformer_blocks.5.attn.to_k_text.weight" in st
    assert "dit.transformer_blocks.5.ff.w2.weight" not in st and "style_encoder.blocks.7.mlp.w1.weight" not in st
    assert "dit.transformer_blocks.5.attn_norm.linear.bias" in st and "style_encoder.blocks.1.mlp.w1.weight" in st
    for net in ("style", "text"):   # the image the encoder blocks [0, 2) leave is x times block 2's norm weight
        assert f"{DS.ENC[net]['prefix']}.2.attention_norm.weight" in st and f"{DS.ENC[net]['prefix']}.2.mlp_norm.weight" not in st


def test_the_stand_in_changes_nothing_while_it_is_off():
    assert DS._ROUND is None
    w = WF.weights("synth")[1]
    cases = [WF.case("blocks", 1, 0, 2, False), WF.case("enc blocks", "text"), WF.case("enc end", "style"), WF.case("cond")]
    with torch.no_grad():
        before = [c.outputs(w) for c in cases]
        with DS.Rounding("f16"):
            on = cases[0].outputs(w)
            with DS.Rounding.off():
                inside = [c.outputs(w) for c in cases]
        assert DS._ROUND is None
        after = [c.outputs(w) for c in cases]
    assert not torch.equal(on["x"], before[0]["x"])
    for a, b, c in zip(before, inside, after):
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    # the site map: Engine::Site by weight name, SITE_COND at split-bf16 under the f16 preset
    for name, site in (("dit.transformer_blocks.3.attn.to_q", "dit_block"), ("dit.transformer_blocks.3.ff.w2", "dit_block"),
                       ("dit.transformer_blocks.3.attn.to_v_text", "cross_kv"), ("dit.transformer_blocks.3.attn_norm.linear", "cond"),
                       ("style_encoder.blocks.2.mlp.w1", "encoder"), ("dit.phoneme_proj", "encoder"), ("style_encoder.out_proj", "encoder"),
                       ("style_encoder.in_proj", "cond"), ("velocity", "cond"), ("dit.norm_out.linear", "cond"), ("dit.emb_proj.0", "cond")):
        assert DS.site_of(name) == site, name
    assert DS.SITE_FMT["f16"]["cond"] == "bf16x3" and DS.SITE_FMT["f16"]["dit_block"] == "f16"


def test_adaln_zero_is_the_identity_in_the_reference():
    w = WF.weights("zero")[1]
    c = WF.case("blocks", 1, 0, 2, False)
    with torch.no_grad():
        out = c.outputs(w)
    assert torch.equal(out["x"], c.x.double()) and not c.table(w).any()
    assert torch.equal(out["img"], DS.layer_norm(c.x.double()))


def _params():
    out = []
    for fam in ("synth",) + WF.FAMILIES:
        for c, prec in WF.bounded_cases(fam):
            out.append(pytest.param(fam, c, prec, id=f"{fam}-{'-'.join(map(str, c.key))}-{prec}"))
    return out


@pytest.mark.parametrize("fam,case,prec", _params())
def test_amplification_stays_under_the_cap_and_operands_in_range(fam, case, prec):
    """A <= 8 on every row and utterance of every metric the GPU test compares; fp16 sites at or below 65504 / 4"""
    A = WF.amplification(fam, case, prec)
    e, amax, _ = WF.e_model(fam, case, prec)
    for m, a in A.items():
        assert torch.isfinite(e[m]).all() and torch.isfinite(a).all(), m
        print(f"[weight families cpu] {fam} {case.key} {prec} {m}: A max {float(a.max()):.2f}, e_model max {float(e[m].max()):.2e}")
        assert float(a.max()) <= WF.A_CAP, f"{m}: A = {float(a.max()):.2f} at index {int(a.argmax())}"
    for site, v in amax.items():
        if DS.SITE_FMT[prec][site] == "f16":
            assert v <= WF.F16_HEADROOM, f"{site}: largest operand {v:.4g}"


# (family, case, slip, metric): the slip must miss BOUND x A + floor by 3x somewhere, against the stand-in's own output
NEAR_MISSES = [
    ("common", ("blocks", 0, 0, 2, False), "fold_term_dropped", "row"),
    ("norms", ("blocks", 1, 0, 2, False), "swap_qk_norm", "row"),
    ("norms", ("enc end", "text"), "k_norm_self", "k"),
    ("norms", ("blocks", 1, 0, 2, False), "abs_head_norm", "row"),
    ("mod", ("blocks", 1, 0, 2, False), "scale_only", "row"),
    ("mod", ("cond",), "no_tanh", "mod"),
    ("colscale", ("blocks", 1, 0, 2, False), "w2_col_shift", "row"),
    ("colscale", ("cond",), "head_col_shift", "head"),
]


@pytest.mark.parametrize("prec", ["bf16x3", "f16"])
@pytest.mark.parametrize("fam,key,slip,metric", NEAR_MISSES, ids=[f"{n[0]}-{n[2]}" for n in NEAR_MISSES])
def test_near_misses_break_the_allowance(fam, key, slip, metric, prec):
    c = WF.case(*key)
    allow, _ = WF.allowance(fam, c, prec)
    stand_in = WF.e_model(fam, c, prec)[2]
    with torch.no_grad():
        wrong = c.outputs(WF.weights(fam)[1], slip=slip)
    ratio = c.errors(stand_in, wrong)[metric] / allow[metric]
    print(f"[weight families cpu] near miss {fam} {slip} {prec}: {float(ratio.max()):.1f}x the allowance")
    assert float(ratio.max()) > 3, f"{slip} under {fam} is within 3x the allowance ({float(ratio.max()):.2f}x)"
