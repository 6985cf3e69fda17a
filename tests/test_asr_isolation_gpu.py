"""GPU: row isolation of the recogniser and the CTC entries, bit for bit, no tolerance (the project's padding rule,
tests/test_padding_gpu.py): a row's logp, nll, ids and n_ids are the same bits alone and inside a ragged batch, with N padded beyond
need, with NaN / garbage behind n_len and outside [p0, p1), on a stale (0xFF) workspace, and run twice."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SEED = 3
C = 198


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0)
    e.load_synthetic(SEED, parts=("asr",))
    e.finalize()
    return e


def run(eng, x, ns, tokens, p0, p1, stale=False):
    """-> per row (logp (4 n, C), nll, ids list) as host arrays; frames behind 4 n must be 0.0, ids behind the count 0"""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(eng.device)
    B, N = x.shape[:2]
    if stale:
        eng._workspace(eng.lib.smtts_asr_workspace_bytes(eng.h, B, N)).fill_(0xFF)
    logp = eng.asr_logprobs(x, ns)
    ts = [4 * n for n in ns]
    nll = eng.ctc_score(logp, ts, torch.from_numpy(np.ascontiguousarray(tokens, np.int32)).to(eng.device), p0, p1)
    ids, n_ids = eng.ctc_greedy(logp, ts)
    torch.cuda.synchronize()
    logp, nll, ids, n_ids = logp.cpu().numpy(), nll.cpu().numpy(), ids.cpu().numpy(), n_ids.cpu().numpy()
    out = []
    for b in range(B):
        assert not logp[b, ts[b]:].any() and not ids[b, n_ids[b]:].any()
        out.append((logp[b, :ts[b]].copy(), nll[b:b + 1].copy(), ids[b, :n_ids[b]].copy()))
    return out


def same(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


@pytest.mark.parametrize("n,L", [(1, 1), (7, 5), (40, 30)])       # 40 frames = 160: across the 56-frame conv tiles and the 64-frame tiles
def test_a_row_keeps_its_bits(eng, n, L):
    g = np.random.default_rng(n)
    row = g.standard_normal((n, 64)).astype(np.float32)
    tok = g.integers(1, C, L).astype(np.int32)
    alone = run(eng, row[None], [n], tok[None], [0], [L])[0]
    assert np.isfinite(alone[0]).all() and np.isfinite(alone[1]).all()
    assert same(alone, run(eng, row[None], [n], tok[None], [0], [L])[0])                       # twice
    assert same(alone, run(eng, row[None], [n], tok[None], [0], [L], stale=True)[0])           # a stale workspace
    # N padded beyond need, NaN behind n_len; the token window inside a longer row of garbage
    N, P, p0 = n + 9, L + 7, 3
    xp = np.full((1, N, 64), np.nan, np.float32)
    xp[0, :n] = row
    tp = np.full((1, P), 2 ** 31 - 1, np.int32)
    tp[0, :p0] = -7
    tp[0, p0:p0 + L] = tok
    assert same(alone, run(eng, xp, [n], tp, [p0], [p0 + L], stale=True)[0])
    # inside a ragged batch: a longer row in front, a shorter one and an empty one behind
    ns = [N, n, max(1, n // 2), 0]
    xb = g.standard_normal((4, N, 64)).astype(np.float32)
    xb[1] = xp[0]
    xb[2, ns[2]:] = np.inf
    tb = g.integers(1, C, (4, P)).astype(np.int32)
    tb[1] = tp[0]
    got = run(eng, xb, ns, tb, [0, p0, 0, 0], [P, p0 + L, 1, 2], stale=True)
    assert same(alone, got[1])
    assert np.isposinf(got[3][1][0]) and got[3][2].size == 0                                   # the empty row: +inf, no ids
    assert same(got[2], run(eng, xb[2:3, :ns[2]], [ns[2]], tb[2:3], [0], [1])[0])
