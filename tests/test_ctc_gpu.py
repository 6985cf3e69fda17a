"""GPU: smtts_ctc_score against F.ctc_loss in fp64 fed the same fp32 log-probabilities, smtts_ctc_greedy against the restatement
(tests/helpers/asr_ref.py), exactly.

The bound is derived, not tuned: |nll - nll64| <= 4 T 2^-24 max(1, |nll64|), from at most four roundings per time step (the two
differences inside the log-sum-exp, its sum, the added emission) on values no larger than |nll|, first order, worst case.  torch's own
fp32 CPU run sits at 2e-8 .. 4.4e-7 relative; the device's figure is printed by every case (MI355X, 2026-10-20: 0 .. 1.9e-7 relative,
4.2e-8 at (900, 198) where 2.1e-4 is allowed)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import asr_ref as R

pytestmark = pytest.mark.gpu
C = 198


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    return HipEngine(0)   # the CTC entries need no weights


def rand_logp(g, B, T, sharp=1.0):
    return (sharp * torch.randn(B, T, C, generator=g)).log_softmax(-1).float()


def ref64(logp, ts, targets):
    """F.ctc_loss(reduction='none', zero_infinity=False) in fp64, row by row (rows with an empty target or no frames: +inf)."""
    out = []
    for b, tgt in enumerate(targets):
        t = int(ts[b])
        if t <= 0 or len(tgt) == 0:
            out.append(np.inf)
            continue
        lp = logp[b, :t].double()[:, None]
        out.append(float(F.ctc_loss(lp, torch.tensor([tgt]), torch.tensor([t]), torch.tensor([len(tgt)]), blank=0, reduction="none",
                                    zero_infinity=False)))
    return np.array(out)


def run(eng, logp, ts, tokens, p0, p1):
    tok = torch.as_tensor(np.asarray(tokens, dtype=np.int32)).to(eng.device)
    nll = eng.ctc_score(logp.to(eng.device).contiguous(), ts, tok, p0, p1)
    torch.cuda.synchronize()
    return nll.cpu().numpy()


def check(nll, want, T, tag):
    for b, (a, w) in enumerate(zip(nll, want)):
        if np.isinf(w):
            assert np.isposinf(a), (tag, b, a, w)
            continue
        bound = 4 * T * 2.0 ** -24 * max(1.0, abs(w))
        print(f"ctc_score {tag} row {b}: nll {a:.6f} vs fp64 {w:.6f}, |diff| {abs(a - w):.3e} (rel {abs(a - w) / max(1.0, abs(w)):.2e}), bound {bound:.3e}")
        assert abs(a - w) <= bound, (tag, b, a, w, bound)


EDGE = [(1, 1, "distinct"), (4, 4, "distinct"), (7, 4, "equal"), (6, 4, "equal"), (395, 198, "equal"), (900, 198, "random")]


@pytest.mark.parametrize("T,L,kind", EDGE)
def test_score_matches_fp64_ctc_loss_at_the_edge_shapes(eng, T, L, kind):
    g = torch.Generator().manual_seed(100 * T + L)
    logp = rand_logp(g, 1, T)
    if kind == "distinct":
        tgt = list(range(3, 3 + L))
    elif kind == "equal":
        tgt = [17] * L
    else:
        tgt = torch.randint(1, C, (L,), generator=g).tolist()
    want = ref64(logp, [T], [tgt])
    if (T, L) == (6, 4):
        assert np.isposinf(want[0])          # infeasible: four equal labels need seven frames
    else:
        assert np.isfinite(want[0])
    nll = run(eng, logp, [T], [tgt], [0], [L])
    check(nll, want, T, f"T{T} L{L} {kind}")


def test_score_defined_edges_in_one_batch(eng):
    """t_len = 0, L = 0, p0 > 0, a window clamped by p1 > P, a negative p0, a token outside [1, C) clamped."""
    g = torch.Generator().manual_seed(5)
    B, T, P = 6, 23, 9
    logp = rand_logp(g, B, T)
    tokens = torch.randint(1, C, (B, P), generator=g).numpy().astype(np.int32)
    tokens[5, 2] = 4000                       # the host's error: clamped to C - 1
    ts = [0, 23, 23, 19, 23, 23]
    p0 = [0, 4, 3, 2, -5, 0]
    p1 = [9, 4, 9, 40, 6, 5]
    targets = []
    for b in range(B):
        a, e = R.clamp_window(p0[b], p1[b], P)
        targets.append([min(max(int(v), 1), C - 1) for v in tokens[b, a:e]])
    want = ref64(logp, ts, targets)
    assert np.isposinf(want[0]) and np.isposinf(want[1]) and np.isfinite(want[2:]).all()
    check(run(eng, logp, ts, tokens, p0, p1), want, T, "edges")


def test_score_with_minus_inf_entries_is_finite_or_inf_never_nan(eng):
    g = torch.Generator().manual_seed(6)
    T, L = 12, 4
    tgt = [5, 9, 9, 30]
    logp = rand_logp(g, 3, T)
    logp[0, :, 77] = -np.inf                  # off the path: no effect
    logp[1, 3, 0] = -np.inf                   # on the path at one frame: other paths remain
    logp[1, 5, 9] = -np.inf
    logp[2, 4, :] = -np.inf                   # a whole frame: nothing remains
    want = ref64(logp, [T] * 3, [tgt] * 3)
    assert np.isfinite(want[:2]).all() and np.isposinf(want[2])
    nll = run(eng, logp, [T] * 3, [tgt] * 3, [0] * 3, [L] * 3)
    assert not np.isnan(nll).any()
    check(nll, want, T, "minus-inf")


def test_score_one_nan_entry_makes_the_row_nan(eng):
    g = torch.Generator().manual_seed(7)
    T, L = 12, 4
    logp = rand_logp(g, 2, T)
    logp[1, 6, 0] = np.nan                    # the blank of a middle frame: every path but one reads it
    nll = run(eng, logp, [T] * 2, [[5, 9, 9, 30]] * 2, [0] * 2, [L] * 2)
    assert np.isfinite(nll[0]) and np.isnan(nll[1])


@pytest.mark.parametrize("N,P", [(12, 5), (225, 198)])
def test_score_prefers_the_spoken_sequence(eng, N, P):
    """logp peaked on a token sequence scores lower against it than against it with one token dropped or replaced."""
    T = 4 * N
    g = torch.Generator().manual_seed(N)
    seq = torch.randint(1, C, (P,), generator=g).tolist()
    for i in range(1, P):                     # no equal neighbours: the planted frames then need no blanks
        if seq[i] == seq[i - 1]:
            seq[i] = seq[i] % (C - 1) + 1
    frames = [seq[min(P - 1, t * P // T)] for t in range(T)]
    logits = torch.randn(1, T, C, generator=g)
    logits[0, torch.arange(T), torch.tensor(frames)] += 8.0
    logp = logits.log_softmax(-1).float()
    dropped = seq[:P // 2] + seq[P // 2 + 1:]
    wrong = seq[P // 2] % (C - 1) + 1
    if wrong in (seq[P // 2 - 1], seq[min(P - 1, P // 2 + 1)]):
        wrong = wrong % (C - 1) + 1
    replaced = seq[:P // 2] + [wrong] + seq[P // 2 + 1:]
    tok = np.zeros((3, P), dtype=np.int32)
    tok[0], tok[1, :P - 1], tok[2] = seq, dropped, replaced
    nll = run(eng, logp.expand(3, T, C).contiguous(), [T] * 3, tok, [0] * 3, [P, P - 1, P])
    print(f"planted N{N} P{P}: nll spoken {nll[0]:.4f}, one dropped {nll[1]:.4f}, one replaced {nll[2]:.4f}")
    assert np.isfinite(nll).all() and nll[0] < nll[1] and nll[0] < nll[2]


def test_greedy_equals_the_restatement_on_planted_rows(eng):
    g = torch.Generator().manual_seed(9)
    B, T = 6, 300
    logp = rand_logp(g, B, T, sharp=3.0)
    logp[1, :, :] = -5.0                      # all ties: class 0 everywhere = an all-blank row
    logp[2, :, 0] = 0.0                       # blank wins every frame
    logp[3, :10] = -9.0
    for t, c in enumerate([4, 4, 0, 4, 7, 7, 7, 0, 0, 9]):   # repeats separated by a blank stay two tokens
        logp[3, t, c] = -0.1
    logp[4, 0, 5] = logp[4, 0, 2] = 1.0       # a tie between 2 and 5: the lower class
    ts = [T, T, T, 10, 1, 257]
    ids, n = eng.ctc_greedy(logp.to(eng.device).contiguous(), ts)
    torch.cuda.synchronize()
    ids, n = ids.cpu().numpy(), n.cpu().numpy()
    for b in range(B):
        want = R.greedy(logp[b].numpy(), ts[b])
        assert n[b] == len(want) and ids[b, :n[b]].tolist() == want and not ids[b, n[b]:].any(), b
    assert n[1] == 0 and n[2] == 0 and ids[3, :3].tolist() == [4, 4, 7] and ids[4, 0] == 2
