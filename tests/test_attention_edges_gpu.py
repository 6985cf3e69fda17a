"""GPU: the three softmax implementations on peaked logits and hard masks, per element against fp64.

attention_img.hip (img:bf16x3 / img:f16 / img:bf16), attention.hip (the fp32 VALU kernel) and align.hip's attn_text_mass run the
case families of tests/helpers/attn_ref.py (A one winner at the positions where indexing goes wrong, B a masked decoy holding the
row's largest logit and V = 1e4, C dead chunks, D anti-aligned keys under a pad position's logit 0, E moderate peaks with ragged
masks) at the smallest shapes at which each path of the kernel exists (attn_ref.CASES).  The assertion is
    |got - as_computed(fmt)| <= bound(fmt)      for EVERY element: no row, head or batch entry left out, no norm over the tensor,
and finite outputs.  as_computed is the operation in fp64 on the operands as the kernel holds them; bound is built from the
reference's own quantities and the format units with one safety factor (attn_ref.SAFETY = 4); tests/test_attn_ref_cpu.py shows
that eight plausible slips break it.  Rows that are masked as queries are compared too: the kernel computes them.

Each item prints one "[attn edges] ... worst error / bound" line (pytest -s).  Measured record (worst error / bound per kernel
over all cases, MI355X; a record, not bars: the assertion is ratio <= 1 with the stated safety factor):
    valu:fp32 0.083 (E case 6)   img:bf16x3 0.339 (A0 case 6)   img:f16 0.611 (E case 6)   img:bf16 0.460 (E case 6)
    tap:bf16x3 0.064 (E case 5)  tap:f16 0.200 (E case 3)      tap:bf16 0.236 (E case 6)
No ratio comes near 1.  f16 and bf16 show no error that as_computed does not model beyond operands held on the neighbouring
format value (attn_ref.tie_slack): the attention bound's P rounding term covers them, the tap bound carries them itself.
"""
import functools

import pytest
import torch

from tests.helpers import attn_ref as R

pytestmark = pytest.mark.gpu

KERNELS = {"valu:fp32": ("fp32", False), "img:bf16x3": ("bf16x3", "img:bf16x3"), "img:f16": ("f16", "img:f16"), "img:bf16": ("bf16", "img:bf16")}
TAP_FMTS = ("bf16x3", "f16", "bf16")
TAP_GRID = [(f, c) for f, c in R.GRID if R.CASES[c][4] > 0]


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    return HipEngine(0, "bf16x3")


@functools.lru_cache(maxsize=None)
def _inputs(family, case):
    return R.build_case(family, case)


@functools.lru_cache(maxsize=None)
def _ref(family, case, fmt):
    """the fp64 reference and its bound: once per (family, shape, format), shared by the tests that need it, never written to"""
    ref = R.as_computed(fmt, *_inputs(family, case)[0])
    return ref.out, R.bound(fmt, ref)


@functools.lru_cache(maxsize=None)
def _tap_ref(family, case, fmt):
    ref = R.tap_as_computed(fmt, *_inputs(family, case)[0])
    return ref.mass, R.tap_bound(ref)


def _worst(got, want, bd):
    """largest error / bound over every element (inf where the bound is 0 and the value differs), and where"""
    err = (got.double() - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bd)        # (bd = 0: exact zeros are demanded)
    ratio = torch.nan_to_num(ratio, nan=float("inf"))
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape)), float(err.flatten()[i])


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("family,case", R.GRID, ids=[f"{f}-case{c}" for f, c in R.GRID])
def test_attention_within_the_bound_everywhere(eng, family, case, kernel):
    fmt, mfma = KERNELS[kernel]
    inp, info = _inputs(family, case)
    want, bd = _ref(family, case, fmt)
    qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt = inp
    got = eng.test_attention(qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt, mfma=mfma).cpu()
    assert got.shape == want.shape
    ratio, at, err = _worst(got, want, bd)
    print(f"\n[attn edges] {family} case {case} {kernel}: worst error / bound = {ratio:.3f} at (b, n, d) = {at} (error {err:.3e})")
    assert bool(torch.isfinite(got).all()), f"{kernel}: non-finite output"
    dead = ~torch.cat([m for m in (ms, mr, mt) if m is not None], 1).any(1)
    assert bool(dead.any()) and not got[dead].any(), "a batch row whose keys are all masked must be exactly 0"
    assert ratio <= 1.0, f"{family} case {case} {kernel}: error / bound = {ratio:.3f} at (b, n, d) = {at} (error {err:.3e})"


@pytest.mark.parametrize("fmt", TAP_FMTS)
@pytest.mark.parametrize("family,case", TAP_GRID, ids=[f"{f}-case{c}" for f, c in TAP_GRID])
def test_text_mass_within_the_bound_everywhere(eng, family, case, fmt):
    inp, info = _inputs(family, case)
    want, bd = _tap_ref(family, case, fmt)
    qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt = inp
    got = eng.test_attn_text_mass(qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt, fmt=fmt).cpu()
    assert got.shape == want.shape
    ratio, at, err = _worst(got, want, bd)
    print(f"\n[attn edges] {family} case {case} tap:{fmt}: worst error / bound = {ratio:.3f} at (b, n, p) = {at} (error {err:.3e})")
    assert bool(torch.isfinite(got).all())
    # the tap's contract: exactly 0 on masked frames and masked text columns, a frame's row sums to at most 1
    assert not got[~ms].any() and not got.transpose(1, 2)[~mt].any()
    assert float(got.sum(-1).max()) <= 1.0 + 1e-6 and float(got.min()) >= 0.0
    if info.winner is not None:      # a text winner takes the frame's whole mass
        T0 = info.L.N + info.L.R
        rows = (info.winner >= T0).all(1) & ms
        if bool(rows.any()):
            idx = (info.winner[:, 0] - T0).clamp_min(0)[..., None]
            assert float((got.gather(2, idx)[..., 0][rows] - 1).abs().max()) <= 1e-5
    assert ratio <= 1.0, f"{family} case {case} tap:{fmt}: error / bound = {ratio:.3f} at (b, n, p) = {at} (error {err:.3e})"
