"""GPU: the recogniser's kernels (smtts_asr_logprobs) against the fp64 helper (tests/helpers/asr_ref.py: every row alone at its own
length), seeded synthetic weights, valid frames only.

The bar.  e32 = the largest |log-prob error| of the SAME helper run in torch fp32 on the CPU against its fp64 run over these cases;
the device must stay within 16 x e32.  The margin is for another summation order and the device's exp / rsqrt through seven layers; a
16-bit operand anywhere would land near 1e-3, two orders outside.  e32 is measured here by the test itself, with the committed recipe.
Measured (MI355X, 2026-10-20; `pytest -s` prints both figures): e32 = 3.04e-6, so the bar is 4.86e-5; the device's worst error 3.97e-6."""
import numpy as np
import pytest
import torch

from tests.helpers import asr_ref as R

pytestmark = pytest.mark.gpu
SEED = 3
CASES = [(1, 1, [1]), (3, 7, [7, 3, 1]), (2, 40, [40, 33]), (1, 225, [225])]


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0)
    e.load_synthetic(SEED, parts=("asr",))
    e.finalize()
    assert e.has("asr") and not e.has("dit")
    return e


@pytest.fixture(scope="module")
def cases():
    """[(x, lengths, fp64 reference, e32 of the case)], computed once"""
    m64, m32 = R.build(SEED), R.build(SEED, torch.float32)
    g = torch.Generator().manual_seed(0)
    out = []
    for B, N, lens in CASES:
        x = torch.randn(B, N, 64, generator=g)
        ref = R.logprobs_rows(m64, x, lens)
        out.append((x, lens, ref, float((R.logprobs_rows(m32, x, lens).double() - ref).abs().max())))
    return out


def test_logprobs_stay_within_16_e32_of_the_fp64_helper(eng, cases):
    e32 = max(c[3] for c in cases)
    assert 5e-7 < e32 < 1e-5, e32            # the helper's own fp32 error is where the issue measured it (1.5e-6 .. 2.6e-6)
    worst = 0.0
    for x, lens, ref, _ in cases:
        got = eng.asr_logprobs(x.to(eng.device), lens)
        torch.cuda.synchronize()
        got = got.cpu().double()
        for b, n in enumerate(lens):
            err = float((got[b, :4 * n] - ref[b, :4 * n]).abs().max())
            worst = max(worst, err)
            assert not got[b, 4 * n:].any()                          # behind the row's end: exactly 0.0
            assert abs(float(got[b, :4 * n].exp().sum(-1).mean()) - 1.0) < 1e-5
    print(f"asr_logprobs: e32 {e32:.3e}, bar 16 e32 = {16 * e32:.3e}, device worst |log-prob error| {worst:.3e}")
    assert worst <= 16 * e32, (worst, e32)


def test_greedy_on_network_outputs_equals_the_restatement(eng, cases):
    x, lens, _, _ = cases[2]
    logp = eng.asr_logprobs(x.to(eng.device), lens)
    ts = [4 * n for n in lens]
    ids, n = eng.ctc_greedy(logp, ts)
    torch.cuda.synchronize()
    lp, ids, n = logp.cpu().numpy(), ids.cpu().numpy(), n.cpu().numpy()
    for b in range(len(lens)):
        want = R.greedy(lp[b], ts[b])
        assert n[b] == len(want) and ids[b, :n[b]].tolist() == want and not ids[b, n[b]:].any()
    assert n.sum() > 0
