"""CPU: the fp64 per-stage statement of the DiT and the condition encoders (oracle/dit_stages.py), which
tests/test_dit_kernels_gpu.py holds each stage's kernels to, composes to the fp32 oracle (oracle/dit_oracle.py) and through it to
the reference's own vectors (tests/golden/)."""
import numpy as np
import pytest
import torch

from oracle import dit_oracle as O
from oracle import dit_stages as DS
from tests.conftest import golden, rel_l2


def _cases():
    g = torch.Generator().manual_seed(3)
    B, N, R, P = 3, 13, 6, 9
    ref = torch.randn(B, R, 64, generator=g)
    ref_len = torch.tensor([R, 1, 4])
    ids = torch.randint(1, 198, (B, P), generator=g)
    ph_mask = torch.ones(B, P, dtype=torch.bool)
    ph_mask[1, 5:] = False
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[2, 9:] = False
    x_t = torch.randn(B, N, 64, generator=g)
    t = torch.tensor([0.0, 0.5, 1.0])
    return ref, ref_len, ids, ph_mask, mask, x_t, t


def test_stage_references_compose_to_the_oracle(dit_weights):
    ref, ref_len, ids, ph_mask, mask, x_t, t = _cases()
    with torch.no_grad():
        want = O.encode_conditions(dit_weights, ref, ref_len, ids, ph_mask)
        got = DS.encode_conditions(dit_weights, ref, ref_len, ids, ph_mask)
        assert torch.equal(got["ref_mask"], want["ref_mask"])
        for k in ("ref_seq", "phoneme_mem", "k_ref", "v_ref", "k_text", "v_text"):
            assert rel_l2(got[k].numpy(), want[k].numpy()) < 2e-5, k
        v_want = O.denoise_step(dit_weights, x_t, mask, t, want, ph_mask=ph_mask)
        v_got = DS.denoise_step(dit_weights, x_t, mask, t, got, ph_mask)
    assert rel_l2(v_got.numpy(), v_want.numpy()) < 2e-5
    # the intermediates the stage tests read one at a time
    tr = {}
    with torch.no_grad():
        O.denoise_step(dit_weights, x_t, mask, t, want, ph_mask=ph_mask, trace=tr)
        x0 = DS.embed(dit_weights, x_t, mask)
        assert rel_l2(x0.numpy(), tr["x0"].numpy()) < 2e-6
        rows = DS.mod_table(dit_weights, t)
        x1 = DS.dit_block(dit_weights, 0, tr["x0"].double(), mask, rows, dict(want, ph_mask=ph_mask))
    assert rel_l2((x1 - tr["x0"].double()).numpy(), (tr["x1"] - tr["x0"]).double().numpy()) < 2e-5


def test_stage_references_match_the_golden_vectors(dit_weights):
    """through dit_oracle's pin: the fp64 stages against the reference modules' own outputs"""
    g = golden("case_small.npz")
    ref, ref_len = torch.from_numpy(g["ref"]), torch.from_numpy(g["ref_len"])
    ids, ph_mask = torch.from_numpy(g["ids"]), torch.from_numpy(g["ph_mask"])
    mask, t, x_t = torch.from_numpy(g["mask"]), torch.from_numpy(g["t"]), torch.from_numpy(g["x_t"])
    with torch.no_grad():
        c = DS.encode_conditions(dit_weights, ref, ref_len, ids, ph_mask)
        assert rel_l2(c["ref_seq"].numpy(), g["ref_seq"]) < 2e-5
        assert rel_l2(DS.embed(dit_weights, x_t, mask).numpy(), g["x_embed"]) < 2e-5
        v = DS.denoise_step(dit_weights, x_t, mask, t, c, ph_mask)
    assert rel_l2(v.numpy(), g["velocity"]) < 2e-5


@pytest.mark.parametrize("variant", ["tap_shift", "no_remask"])
def test_conv_near_misses_differ(dit_weights, variant):
    """the near-miss references the GPU test uses for its power check are not the same function as the reference"""
    _, _, _, _, mask, x_t, _ = _cases()
    with torch.no_grad():
        a = DS.embed(dit_weights, x_t, mask)
        b = DS.embed(dit_weights, x_t, mask, tap_shift=1) if variant == "tap_shift" else DS.embed(dit_weights, x_t, mask, remask=False)
    assert rel_l2(b.numpy(), a.numpy()) > 1e-3
