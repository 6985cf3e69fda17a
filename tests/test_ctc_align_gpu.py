"""GPU: smtts_ctc_align against its numpy float32 restatement (tests/helpers/ctc_align_ref.py, itself held to a brute force by
tests/test_ctc_align_cpu.py): spans, frame_tok and the BITS of tok_logp and score.  Every step of the definition is a single fp32
operation in a fixed order, so there is no tolerance anywhere but in the comparison with smtts_ctc_score, whose own bound is used.
Then a planted segmentation that does not go through the restatement, row isolation bit for bit, the entry between guard bands
(tests/helpers/guarded.py) and every refused argument."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import ctc_align_ref as R
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
NC = 198


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    return HipEngine(0)   # the CTC entries need no weights


def rand_logp(g, B, T, nc=NC, sharp=1.0):
    return (sharp * torch.randn(B, T, nc, generator=g)).log_softmax(-1).float()


def run(eng, logp, ts, tokens, p0, p1, frames=True):
    tok = torch.as_tensor(np.ascontiguousarray(tokens, dtype=np.int32)).to(eng.device)
    out = eng.ctc_align(torch.as_tensor(logp).to(eng.device).contiguous(), ts, tok, p0, p1, frames=frames)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def same_bits(a, b):
    """float32 arrays equal bit for bit; a NaN equals a NaN (its payload is the adder's business, not the definition's)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes()


def same(got, logp, ts, tokens, p0, p1, tag):
    """spans, tok_logp (bits), score (bits) and frame_tok equal the restatement's."""
    want = R.align_batch(np.asarray(logp), ts, np.asarray(tokens), p0, p1)
    spans, tok_logp, score = got[:3]
    assert spans.dtype == np.int32 and tok_logp.dtype == np.float32 and score.dtype == np.float32
    assert np.array_equal(spans, want[0]), (tag, "spans")
    assert same_bits(tok_logp, want[1]), (tag, "tok_logp", tok_logp, want[1])
    assert same_bits(score, want[3]), (tag, "score", score, want[3])
    if len(got) > 3:
        assert got[3].dtype == np.int32 and np.array_equal(got[3], want[2]), (tag, "frame_tok")
    return want


def tokens_for(g, T, L, kind):
    if kind == "repeat":
        return [17] * L
    tok = torch.randint(1, NC, (L,), generator=g).tolist()
    if kind == "tight":                                        # no equal neighbours: feasible at T == L
        for i in range(1, L):
            if tok[i] == tok[i - 1]:
                tok[i] = tok[i] % (NC - 1) + 1
    return tok


SHAPES = [(1, 1, "random"), (2, 1, "random"), (3, 2, "repeat"), (2, 2, "repeat"), (17, 5, "random"), (33, 16, "random"),
          (160, 40, "random"), (900, 198, "random"), (1024, 198, "random")]   # the last: the entry's limits, all 125 248 bytes of LDS


@pytest.mark.parametrize("T,L,kind", SHAPES)
def test_equals_the_restatement_at_the_edge_shapes(eng, T, L, kind):
    g = torch.Generator().manual_seed(1000 * T + L)
    logp = rand_logp(g, 1, T, sharp=2.0)
    tok = [tokens_for(g, T, L, kind)]
    want = same(run(eng, logp, [T], tok, [0], [L]), logp, [T], tok, [0], [L], (T, L, kind))
    if (T, L) == (2, 2):
        assert np.isneginf(want[3][0]) and (want[0] == -1).all()          # two equal labels need three frames
    else:
        assert np.isfinite(want[3][0]) and (want[0][0, :L] >= 0).all()
        fr = want[2][0]
        assert [int(v) for i, v in enumerate(fr) if v >= 0 and (i == 0 or fr[i - 1] != v)] == list(range(L))   # every token, in order


@pytest.mark.parametrize("T", [17, 160])
def test_ragged_batch_windows_and_clamps(eng, T):
    """t_len = (T, T - 5, 0), windows p0 = (0, 2, P); a fourth row with L = 0 and a fifth with tokens 0 and C + 5 (clamped) and a
    window given as (-3, P + 9)."""
    g = torch.Generator().manual_seed(T)
    B, P = 5, 6
    logp = rand_logp(g, B, T, sharp=2.0)
    tokens = torch.randint(1, NC, (B, P), generator=g).numpy().astype(np.int32)
    tokens[4, 1], tokens[4, 3] = 0, NC + 5
    ts, p0, p1 = [T, T - 5, 0, T, T], [0, 2, P, 3, -3], [P, P, P, 3, P + 9]
    got = run(eng, logp, ts, tokens, p0, p1)
    same(got, logp, ts, tokens, p0, p1, ("ragged", T))
    spans, tok_logp, score, frame_tok = got
    assert np.isfinite(score[[0, 1, 4]]).all() and np.isneginf(score[[2, 3]]).all()
    assert (spans[1, :2] == -1).all() and (spans[1, 2:] >= 0).all() and (spans[2:4] == -1).all() and not tok_logp[2:4].any()
    assert (frame_tok[1, T - 5:] == -1).all() and (frame_tok[2:4] == -1).all() and frame_tok[1].max() == P - 1 and frame_tok[1][frame_tok[1] >= 0].min() == 2
    clamped = tokens[4].copy()
    clamped[1], clamped[3] = 1, NC - 1
    again = run(eng, logp[4:], [T], clamped[None], [0], [P])
    assert all(a[0].tobytes() == b[4].tobytes() for a, b in zip(again, got))


def test_quantised_logp_ties_everywhere(eng):
    """logp in multiples of 0.25: every sum is exact and equal sums are everywhere, so the strict comparisons decide the path."""
    g = torch.Generator().manual_seed(11)
    B, T, P = 4, 28, 7
    logp = torch.round(rand_logp(g, B, T, nc=5, sharp=0.5) * 4.0) / 4.0
    tokens = torch.randint(1, 5, (B, P), generator=g).numpy().astype(np.int32)
    tokens[3] = 2                                              # all equal: a blank between every pair
    got = run(eng, logp, [T] * B, tokens, [0] * B, [P] * B)
    want = same(got, logp, [T] * B, tokens, [0] * B, [P] * B, "quantised")
    other = np.stack([R.align(logp[b].numpy(), T, tokens[b], 0, P, ties="move")["spans"] for b in range(B)])
    assert not np.array_equal(other, want[0])                  # the other tie rule gives other spans on this data: the case can tell


def test_minus_inf_and_nan_entries(eng):
    g = torch.Generator().manual_seed(12)
    T, P = 20, 4
    tok = np.asarray([[5, 9, 9, 30]] * 6, np.int32)
    logp = rand_logp(g, 1, T, sharp=2.0).repeat(6, 1, 1)
    logp[1, :, 77] = -np.inf                                   # a class no label reads
    logp[2, 3, 0] = logp[2, 5, 9] = -np.inf                    # on some paths: others remain
    logp[3, 4, :] = -np.inf                                    # a whole frame: nothing remains
    logp[4, :, 77] = np.nan                                    # NaN in a class no label reads: the result is row 0's
    logp[5, 6, 9] = np.nan                                     # NaN in a class two labels read: whatever the definition gives
    got = run(eng, logp, [T] * 6, tok, [0] * 6, [P] * 6)
    same(got, logp, [T] * 6, tok, [0] * 6, [P] * 6, "inf / nan")
    spans, tok_logp, score, frame_tok = got
    for b in (1, 4):
        assert all(o[b].tobytes() == o[0].tobytes() for o in got), b
    assert np.isfinite(score[2]) and score[2] <= score[0] and np.isneginf(score[3]) and (spans[3] == -1).all() and (frame_tok[3] == -1).all()


def test_frame_tok_null_changes_nothing_else(eng):
    g = torch.Generator().manual_seed(13)
    T, P = 33, 6
    logp, tok = rand_logp(g, 2, T), torch.randint(1, NC, (2, P), generator=g).numpy()
    a = run(eng, logp, [T, 20], tok, [0, 1], [P, P], frames=True)
    b = run(eng, logp, [T, 20], tok, [0, 1], [P, P], frames=False)
    assert len(b) == 3 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("T,P", [(28, 5), (900, 198)])
def test_planted_segmentation_is_found_exactly(eng, T, P):
    """Independent of the restatement: lp = 0 on every token's planted frames and on blank in the planted gaps, -20 elsewhere; the
    only path of score 0 is the planted one."""
    g = torch.Generator().manual_seed(T)
    tok = tokens_for(g, T, P, "random")
    cuts = np.sort(torch.randperm(T - 1, generator=g)[:2 * P - 1].numpy() + 1)
    bounds = [0] + cuts.tolist() + [T]                         # token i on [bounds[2 i], bounds[2 i + 1]), a blank gap behind it
    plan = [(bounds[2 * i], bounds[2 * i + 1] - 1) for i in range(P)]
    logp = torch.full((1, T, NC), -20.0)
    logp[0, :, 0] = 0.0
    for (a, b), c in zip(plan, tok):
        logp[0, a:b + 1, 0] = -20.0
        logp[0, a:b + 1, c] = 0.0
    spans, tok_logp, score, frame_tok = run(eng, logp, [T], [tok], [0], [P])
    assert spans[0].tolist() == [list(ab) for ab in plan]
    assert score[0] == 0.0 and not tok_logp.any()
    want_ft = np.full(T, -1)
    for i, (a, b) in enumerate(plan):
        want_ft[a:b + 1] = i
    assert np.array_equal(frame_tok[0], want_ft)


@pytest.mark.parametrize("T,L", [(4, 2), (28, 7), (160, 40)])
def test_best_path_is_below_the_ctc_score_and_rows_are_isolated(eng, T, L):
    """score <= -nll of smtts_ctc_score on the same buffers, within that entry's own bound 4 T 2^-24 max(1, |nll|).  And bit for bit: a
    row alone, inside the ragged batch, with T padded, with NaN and garbage behind t_len, and twice in a row."""
    g = torch.Generator().manual_seed(7 * T + L)
    P = L + 2
    logp = rand_logp(g, 3, T, sharp=2.0)
    tokens = torch.randint(1, NC, (3, P), generator=g).numpy().astype(np.int32)
    ts, p0, p1 = [T, max(T - 5, 0), 0], [1, 2, P], [1 + L, P, P]
    dev = eng.device
    lp_d, tok_d = logp.to(dev), torch.from_numpy(tokens).to(dev)
    first = eng.ctc_align(lp_d, ts, tok_d, p0, p1, frames=True)
    second = eng.ctc_align(lp_d, ts, tok_d, p0, p1, frames=True)
    nll = eng.ctc_score(lp_d, ts, tok_d, p0, p1)
    torch.cuda.synchronize()
    batch = [o.cpu().numpy() for o in first]
    assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip(batch, second))
    nll = nll.cpu().numpy().astype(np.float64)
    for b in range(3):
        s = float(batch[2][b])
        if np.isinf(nll[b]):
            assert np.isneginf(s), (b, s)
            continue
        bound = 4 * T * 2.0 ** -24 * max(1.0, abs(nll[b]))
        print(f"ctc_align T{T} L{L} row {b}: best path {s:.6f}, -nll {-nll[b]:.6f}, bound {bound:.3e}")
        assert s <= -nll[b] + bound, (b, s, nll[b])
    for b in (0, 1):
        alone = run(eng, logp[b:b + 1], ts[b:b + 1], tokens[b:b + 1], p0[b:b + 1], p1[b:b + 1])
        assert all(a[0].tobytes() == o[b].tobytes() for a, o in zip(alone, batch)), ("alone", b)
        pad = torch.full((1, T + 11, NC), float("nan"))
        pad[0, :, ::3] = 1e30                                  # garbage and NaN behind t_len, in a row of another length
        pad[0, :ts[b]] = logp[b, :ts[b]]
        padded = run(eng, pad, ts[b:b + 1], tokens[b:b + 1], p0[b:b + 1], p1[b:b + 1])
        for a, o in zip(padded[:3], batch[:3]):
            assert a[0].tobytes() == o[b].tobytes(), ("padded", b)
        assert np.array_equal(padded[3][0, :T], batch[3][b]) and (padded[3][0, T:] == -1).all()


@pytest.mark.parametrize("B,T,P,lens,skew", [(1, 1, 1, [1], 0), (3, 17, 5, [17, 12, 0], 4), (2, 33, 16, [33, 30], 0), (1, 900, 198, [900], 4)])
def test_between_guard_bands(eng, B, T, P, lens, skew):
    g = torch.Generator().manual_seed(T + P)
    a = Arena(eng.device)
    lp = a.put("logp", rand_logp(g, B, T), skew=skew)
    tl = a.put("t_len", torch.tensor(lens, dtype=torch.int32))
    tok = a.put("tokens", torch.randint(1, NC, (B, P), generator=g).to(torch.int32), skew=skew)
    p0, p1 = a.put("p0", torch.zeros(B, dtype=torch.int32)), a.put("p1", torch.full((B,), P, dtype=torch.int32))
    spans, tok_logp = a.alloc("spans", (B, P, 2), torch.int32, skew=skew), a.alloc("tok_logp", (B, P), torch.float32, skew=skew)
    frame_tok, score = a.alloc("frame_tok", (B, T), torch.int32, skew=skew), a.alloc("score", (B,), torch.float32, skew=skew)
    call = lambda: eng.lib.smtts_ctc_align(eng.h, eng._stream(), p(lp), p(tl), p(tok), p(p0), p(p1), B, T, P, NC, p(spans), p(tok_logp),
                                           p(frame_tok), p(score))
    ins = {n: b.view.clone() for n, b in a.bufs.items() if b.role == "in"}
    outs, snaps = ["spans", "tok_logp", "frame_tok", "score"], []
    for byte in (0x00, 0xFF):
        a.paint(byte)
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0
        a.assert_clean("smtts_ctc_align", f"{B}x{T}x{P} skew {skew} (guards 0x{byte:02X})")
        snaps.append({n: a[n].clone().cpu().numpy() for n in outs})
    for n in outs:
        assert snaps[0][n].tobytes() == snaps[1][n].tobytes(), n
    for n, t in ins.items():
        assert a[n].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), (n, "an input changed")
    same([snaps[0][n] for n in ("spans", "tok_logp", "score", "frame_tok")], lp.cpu().numpy(), lens, tok.cpu().numpy(), [0] * B, [P] * B, "guarded")


def test_refused_arguments_name_the_entry_and_enqueue_nothing(eng):
    dev = eng.device
    B, T, P = 2, 20, 4
    lp = torch.randn(B, T, NC, device=dev).log_softmax(-1)
    tok = torch.ones(B, P, dtype=torch.int32, device=dev)
    tab = torch.tensor([[20, 12], [0, 0], [4, 4]], dtype=torch.int32, device=dev)
    spans = torch.full((B, P, 2), -7, dtype=torch.int32, device=dev)
    tok_logp, score = torch.full((B, P), -7.0, device=dev), torch.full((B,), -7.0, device=dev)
    frame_tok = torch.full((B, T), -7, dtype=torch.int32, device=dev)

    def align(h=eng.h, lp=lp, tl=tab[0], tok=tok, p0=tab[1], p1=tab[2], B=B, T=T, P=P, Cn=NC, spans=spans, tok_logp=tok_logp,
              frame_tok=frame_tok, score=score):
        return eng.lib.smtts_ctc_align(h, eng._stream(), p(lp), p(tl), p(tok), p(p0), p(p1), B, T, P, Cn, p(spans), p(tok_logp), p(frame_tok),
                                       p(score))

    for kw in (dict(B=0), dict(B=65537), dict(T=0), dict(T=1025), dict(P=0), dict(P=199), dict(Cn=1), dict(Cn=257), dict(lp=None),
               dict(tl=None), dict(tok=None), dict(p0=None), dict(p1=None), dict(spans=None), dict(tok_logp=None), dict(score=None)):
        assert align(**kw) == 1 and b"smtts_ctc_align" in eng.lib.smtts_last_error(eng.h), kw
    assert align(h=None) == 1 and b"smtts_ctc_align" in eng.lib.smtts_last_error(None)
    torch.cuda.synchronize()
    assert bool((spans == -7).all()) and bool((tok_logp == -7).all()) and bool((score == -7).all()) and bool((frame_tok == -7).all())
    assert align() == 0 and align(frame_tok=None) == 0         # ... and the same buffers with good arguments run, with and without frame_tok
    torch.cuda.synchronize()
    assert np.isfinite(score.cpu().numpy()).all() and bool((spans >= 0).all())
    # the Python face
    for bad in (lp.double(), lp[:, :, ::2], lp.cpu(), lp[0]):
        with pytest.raises(ValueError, match="ctc_align: logp"):
            eng.ctc_align(bad, [20, 12], tok, [0, 0], [4, 4])
    for bad in (tok.long(), tok[:1], tok[:, ::2], tok.cpu()):
        with pytest.raises(ValueError, match="ctc_align: tokens"):
            eng.ctc_align(lp, [20, 12], bad, [0, 0], [4, 4])
    with pytest.raises(ValueError, match="outside the supported range"):
        eng.ctc_align(torch.zeros(1, 1025, 4, device=dev), [5], tok[:1], [0], [4])
    with pytest.raises(ValueError, match="outside the supported range"):
        eng.ctc_align(lp, [20, 12], torch.ones(B, 199, dtype=torch.int32, device=dev), [0, 0], [4, 4])
    with pytest.raises(ValueError, match="one frame count"):
        eng.ctc_align(lp, [20], tok, [0, 0], [4, 4])
