"""GPU: row isolation of the verifier entries, bit for bit, no tolerance (the project's padding rule,
tests/test_padding_gpu.py): a row's emb and cos are the same bits alone and inside a ragged batch, with N padded beyond need, with
NaN / garbage behind n_len, on a stale (0xFF) workspace, and run twice."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 5


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0)
    e.load_synthetic(SEED, parts=("sv",))
    e.finalize()
    return e


@pytest.fixture(scope="module")
def voice(eng):
    """one reference embedding every case is compared against"""
    g = torch.Generator().manual_seed(99)
    return eng.sv_embed(torch.randn(1, 30, 64, generator=g).to(eng.device), [30]).clone()


def run(eng, voice, x, ns, stale=False):
    """-> per row (emb (192), cos (1)) as host arrays"""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(eng.device)
    B, N = x.shape[:2]
    if stale:
        eng._workspace(eng.lib.smtts_sv_workspace_bytes(eng.h, B, N)).fill_(0xFF)
    emb = eng.sv_embed(x, ns)
    cos = eng.sv_cosine(emb, voice, B)                     # the whole batch is one group: every row against the one reference
    torch.cuda.synchronize()
    emb, cos = emb.cpu().numpy(), cos.cpu().numpy()
    return [(emb[b].copy(), cos[b:b + 1].copy()) for b in range(B)]


def same(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


@pytest.mark.parametrize("n", [6, 7, 40, 225])            # 225: four frame tiles of sv_tdnn, sixteen blocks of sv_res2net
def test_a_row_keeps_its_bits(eng, voice, n):
    g = np.random.default_rng(n)
    row = g.standard_normal((n, 64)).astype(np.float32)
    alone = run(eng, voice, row[None], [n])[0]
    assert np.isfinite(alone[0]).all() and alone[0].any() and np.isfinite(alone[1]).all() and 0.0 < abs(float(alone[1][0])) < 1.0
    assert same(alone, run(eng, voice, row[None], [n])[0])                        # twice
    assert same(alone, run(eng, voice, row[None], [n], stale=True)[0])            # a stale workspace
    # N padded beyond need (inside the entry's N <= 225), NaN behind n_len
    N = min(n + 9, 225)
    xp = np.full((1, N, 64), np.nan, np.float32)
    xp[0, :n] = row
    if N > n:
        assert same(alone, run(eng, voice, xp, [n], stale=True)[0])
    # inside a ragged batch: a full row in front, a shorter one, a row too short for an embedding and an empty one behind
    ns = [N, n, max(6, n // 2), 3, 0]
    xb = g.standard_normal((5, N, 64)).astype(np.float32)
    xb[1] = xp[0]
    xb[2, ns[2]:] = np.inf
    xb[3, 3:] = np.nan
    xb[4] = np.nan
    got = run(eng, voice, xb, ns, stale=True)
    assert same(alone, got[1])
    for b in (3, 4):                                                              # no embedding: 0.0, and a cosine of 0.0
        assert not got[b][0].any() and got[b][1][0] == 0.0
    assert same(got[2], run(eng, voice, xb[2:3, :ns[2]], [ns[2]])[0])
