"""GPU: smtts_ctc_align_long.  Its definition is smtts_ctc_align's, so wherever both entries accept a call the four outputs
are compared BIT FOR BIT with that entry's; past its limits they are compared, again bit for bit, with the numpy float32 restatement
(tests/helpers/ctc_align_long_ref.py, held to tests/helpers/ctc_align_ref.py by tests/test_ctc_align_long_cpu.py).  No tolerance
anywhere: every step of the definition is a single fp32 operation in a fixed order.  The edge shapes follow from the kernel's own
constants, named here: K states per thread, G steps per trace chunk, CH steps per ring half.  Then a planted segmentation at the
entry's limits that does not go through any restatement, row isolation bit for bit over stale workspace bytes, the entry between guard
bands (tests/helpers/guarded.py) and every refused argument."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import ctc_align_long_ref as R
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
NC = 198
K, G, CH = 32, 256, 8            # smalltts_amd/csrc/ctc_long.hip: CL_K, CL_G, CL_CH
MAX_B, MAX_T, MAX_P = 64, 65536, 16383


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    return HipEngine(0)   # the CTC entries need no weights


def rand_logp(g, B, T, nc=NC, sharp=1.0):
    return (sharp * torch.randn(B, T, nc, generator=g)).log_softmax(-1).float()


def run(eng, logp, ts, tokens, p0, p1, frames=True, entry="ctc_align_long"):
    tok = torch.as_tensor(np.ascontiguousarray(tokens, dtype=np.int32)).to(eng.device)
    out = getattr(eng, entry)(torch.as_tensor(logp).to(eng.device).contiguous(), ts, tok, p0, p1, frames=frames)
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
    assert same_bits(tok_logp, want[1]), (tag, "tok_logp")
    assert same_bits(score, want[3]), (tag, "score", score, want[3])
    if len(got) > 3:
        assert got[3].dtype == np.int32 and np.array_equal(got[3], want[2]), (tag, "frame_tok")
    return want


def same_as_short(eng, logp, ts, tokens, p0, p1, tag):
    """all four outputs of smtts_ctc_align_long equal smtts_ctc_align's on the same call, bit for bit"""
    long_, short = run(eng, logp, ts, tokens, p0, p1), run(eng, logp, ts, tokens, p0, p1, entry="ctc_align")
    assert len(long_) == len(short) == 4
    for name, a, b in zip(("spans", "tok_logp", "score", "frame_tok"), long_, short):
        assert a.dtype == b.dtype and a.shape == b.shape, (tag, name)
        assert same_bits(a, b) if a.dtype == np.float32 else np.array_equal(a, b), (tag, name)
    return long_


def tokens_for(g, L, kind, nc=NC):
    if kind == "repeat":
        return [17] * L
    tok = torch.randint(1, nc, (L,), generator=g).tolist()
    if kind == "tight":                                        # no equal neighbours: feasible at T == L
        for i in range(1, L):
            if tok[i] == tok[i - 1]:
                tok[i] = tok[i] % (nc - 1) + 1
    return tok


# ---- equal to smtts_ctc_align wherever both accept the call ---------------------------------------------------------------------------
SHAPES = [(1, 1, "random"), (2, 1, "random"), (3, 2, "repeat"), (2, 2, "repeat"), (17, 5, "random"), (33, 16, "random"),
          (160, 40, "random"), (900, 198, "random"), (1024, 198, "random")]   # that entry's own test shapes, its limits last


@pytest.mark.parametrize("T,L,kind", SHAPES)
def test_equals_ctc_align_at_its_own_shapes(eng, T, L, kind):
    g = torch.Generator().manual_seed(1000 * T + L)
    logp = rand_logp(g, 1, T, sharp=2.0)
    tok = [tokens_for(g, L, kind)]
    spans, tok_logp, score, frame_tok = same_as_short(eng, logp, [T], tok, [0], [L], (T, L, kind))
    if (T, L) == (2, 2):
        assert np.isneginf(score[0]) and (spans == -1).all() and (frame_tok == -1).all() and not tok_logp.any()
    else:
        assert np.isfinite(score[0]) and (spans[0, :L] >= 0).all()
        fr = frame_tok[0]
        assert [int(v) for i, v in enumerate(fr) if v >= 0 and (i == 0 or fr[i - 1] != v)] == list(range(L))   # every token, in order


@pytest.mark.parametrize("T", [17, 160])
def test_equals_ctc_align_on_the_ragged_batch_with_windows_and_clamps(eng, T):
    """t_len = (T, T - 5, 0), windows p0 = (0, 2, P); a fourth row with L = 0 and a fifth with tokens 0 and C + 5 (clamped) and a
    window given as (-3, P + 9)."""
    g = torch.Generator().manual_seed(T)
    B, P = 5, 6
    logp = rand_logp(g, B, T, sharp=2.0)
    tokens = torch.randint(1, NC, (B, P), generator=g).numpy().astype(np.int32)
    tokens[4, 1], tokens[4, 3] = 0, NC + 5
    ts, p0, p1 = [T, T - 5, 0, T, T], [0, 2, P, 3, -3], [P, P, P, 3, P + 9]
    spans, tok_logp, score, frame_tok = same_as_short(eng, logp, ts, tokens, p0, p1, ("ragged", T))
    assert np.isfinite(score[[0, 1, 4]]).all() and np.isneginf(score[[2, 3]]).all()
    assert (spans[1, :2] == -1).all() and (spans[1, 2:] >= 0).all() and (spans[2:4] == -1).all() and not tok_logp[2:4].any()
    assert (frame_tok[1, T - 5:] == -1).all() and (frame_tok[2:4] == -1).all() and frame_tok[1].max() == P - 1


# ---- equal to the restatement where the new machinery can first go wrong ----------------------------------------------------------------
@pytest.mark.parametrize("half", [0, 1])
def test_every_state_count_across_the_first_thread_boundaries(eng, half):
    """Rows with L = 1 ... 4 K tokens (S = 3 ... 8 K + 1: every odd state count over the first eight threads), T = L + 5, ragged in one
    table of width 4 K.  The entry takes 64 rows per call, so the 4 K = 128 rows are two launches."""
    g = torch.Generator().manual_seed(40 + half)
    B, P = 2 * K, 4 * K
    Ls = list(range(1 + half * B, 1 + (half + 1) * B))
    T = P + 5
    logp = rand_logp(g, B, T, nc=12, sharp=2.0)
    tokens = np.stack([tokens_for(g, P, "tight", nc=12) for _ in range(B)]).astype(np.int32)
    ts = [L + 5 for L in Ls]
    p0 = [(P - L) // 2 if b % 3 == 0 else 0 for b, L in enumerate(Ls)]       # every third row: a window inside the table
    p1 = [a + L for a, L in zip(p0, Ls)]
    same(run(eng, logp, ts, tokens, p0, p1), logp, ts, tokens, p0, p1, ("thread boundaries", half))


@pytest.mark.parametrize("L", [32 * K - 1, 32 * K, 32 * K + 1])
def test_state_count_across_a_wave_boundary(eng, L):
    """S = 2 L + 1 at 64 K - 1, 64 K + 1 and 64 K + 3: the last state in the last thread of wave 0, then in the first of wave 1."""
    g = torch.Generator().manual_seed(L)
    T = L + 5
    logp = rand_logp(g, 1, T, nc=9, sharp=2.0)
    tok = [tokens_for(g, L, "tight", nc=9)]
    want = same(run(eng, logp, [T], tok, [0], [L]), logp, [T], tok, [0], [L], ("wave boundary", L))
    assert np.isfinite(want[3][0])


@pytest.mark.parametrize("T", [G - 1, G, G + 1, G + 2, 2 * G + 1, 2 * G + 2, CH - 1, CH, CH + 1, 2 * CH - 1, 2 * CH, 2 * CH + 1])
def test_frame_counts_at_the_trace_chunk_and_at_the_ring_half(eng, T):
    """The trace walks the steps T - 1 ... 1 in chunks of G: T = G + 1 is exactly one chunk, 2 G + 1 exactly two.  The emission ring turns
    every CH steps.  Two rows: the full length and one frame less; 20 tokens (S = 41: two threads)."""
    g = torch.Generator().manual_seed(T)
    P = min(20, T - 1)
    logp = rand_logp(g, 2, T, sharp=2.0)
    tokens = np.stack([tokens_for(g, P, "tight") for _ in range(2)]).astype(np.int32)
    same(run(eng, logp, [T, T - 1], tokens, [0, 0], [P, P]), logp, [T, T - 1], tokens, [0, 0], [P, P], ("T", T))


@pytest.mark.parametrize("T,L", [(1025, 40), (600, 199), (4100, 1100)])
def test_just_past_the_old_limits_and_one_mid_size_row(eng, T, L):
    g = torch.Generator().manual_seed(T + L)
    nc = NC if T < 4000 else 24
    logp = rand_logp(g, 1, T, nc=nc, sharp=2.0)
    tok = [tokens_for(g, L, "random", nc=nc)]
    want = same(run(eng, logp, [T], tok, [0], [L]), logp, [T], tok, [0], [L], (T, L))
    assert np.isfinite(want[3][0]) and (want[0][0] >= 0).all()


def test_quantised_logp_ties_everywhere(eng):
    """logp in multiples of 0.25: every sum is exact and equal sums are everywhere, so the strict comparisons decide the path.  70 tokens:
    S = 141, the ties cross four thread boundaries."""
    g = torch.Generator().manual_seed(11)
    B, T, P = 4, 300, 70
    logp = torch.round(rand_logp(g, B, T, nc=5, sharp=0.5) * 4.0) / 4.0
    tokens = torch.randint(1, 5, (B, P), generator=g).numpy().astype(np.int32)
    tokens[3] = 2                                              # all equal: a blank between every pair
    same(run(eng, logp, [T] * B, tokens, [0] * B, [P] * B), logp, [T] * B, tokens, [0] * B, [P] * B, "quantised")


def test_minus_inf_and_nan_entries(eng):
    g = torch.Generator().manual_seed(12)
    T, P = 120, 40
    tok = np.asarray([tokens_for(g, P, "tight", nc=60)] * 6, np.int32)
    tok[:, 20] = tok[:, 19] = 9
    logp = rand_logp(g, 1, T, sharp=2.0).repeat(6, 1, 1)
    logp[1, :, 77] = -np.inf                                   # a class no label reads
    logp[2, 3, 0] = logp[2, 50, 9] = -np.inf                   # on some paths: others remain
    logp[3, 60, :] = -np.inf                                   # a whole frame: nothing remains
    logp[4, :, 77] = np.nan                                    # NaN in a class no label reads: the result is row 0's
    logp[5, 60, 9] = np.nan                                    # NaN in a class two labels read: whatever the definition gives
    got = run(eng, logp, [T] * 6, tok, [0] * 6, [P] * 6)
    same(got, logp, [T] * 6, tok, [0] * 6, [P] * 6, "inf / nan")
    spans, tok_logp, score, frame_tok = got
    for b in (1, 4):
        assert all(o[b].tobytes() == o[0].tobytes() for o in got), b
    assert np.isfinite(score[2]) and score[2] <= score[0] and np.isneginf(score[3]) and (spans[3] == -1).all() and (frame_tok[3] == -1).all()


def test_repeated_tokens_switch_the_skip_off_across_a_thread_boundary(eng):
    """State 2 j + 1 may skip the blank in front of it unless tokens j - 1 and j are equal.  Tokens 15 / 16 are the states 31 / 33: the
    last label state of thread 0 and the first of thread 1 (and 31 / 32: threads 1 and 2).  Row 0 has them equal, row 1 different, row
    2 is one token repeated; the frames are so few that the path needs every skip it may take."""
    g = torch.Generator().manual_seed(14)
    P = 2 * K + 8
    base = tokens_for(g, P, "tight", nc=30)
    eq, ne = list(base), list(base)
    eq[K // 2] = eq[K // 2 - 1]
    eq[K] = eq[K - 1]
    T = P + 4
    tokens = np.asarray([eq, ne, [17] * P], np.int32)
    logp = rand_logp(g, 3, 2 * P + 1, nc=30, sharp=2.0)
    ts = [T, T, 2 * P + 1]
    want = same(run(eng, logp, ts, tokens, [0] * 3, [P] * 3), logp, ts, tokens, [0] * 3, [P] * 3, "repeats")
    assert np.isfinite(want[3]).all() and not np.array_equal(want[0][0], want[0][1])
    tight = same(run(eng, logp[:2], [P + 1] * 2, tokens[:2], [0] * 2, [P] * 2), logp[:2], [P + 1] * 2, tokens[:2], [0] * 2, [P] * 2, "repeats, tight")
    assert np.isneginf(tight[3][0]) and np.isfinite(tight[3][1])          # two repeats need two blanks: P + 2 frames


def test_frame_tok_null_changes_nothing_else(eng):
    g = torch.Generator().manual_seed(13)
    T, P = 300, 60
    logp, tok = rand_logp(g, 2, T), torch.randint(1, NC, (2, P), generator=g).numpy()
    a = run(eng, logp, [T, 200], tok, [0, 1], [P, P], frames=True)
    b = run(eng, logp, [T, 200], tok, [0, 1], [P, P], frames=False)
    assert len(b) == 3 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- a planted segmentation at the limits, independent of any restatement -----------------------------------------------------------
def _planted(kind, seed, T, P, nc):
    """-> (logp (T, nc): 0 on the planted path and -10 elsewhere, tokens, spans (P, 2), frame_tok (T,)).  Neighbouring tokens differ, so
    the path needs no blank between them.  "random": token i on a random run of frames, a blank gap behind every token; "earliest":
    token i on frame i alone, blanks behind the last; "latest": blanks first, token i on frame T - P + i."""
    tok = 1 + np.arange(P) % (nc - 1)
    if kind == "random":
        rng = np.random.default_rng(seed)
        bounds = np.concatenate(([0], np.sort(rng.choice(T - 1, 2 * P - 1, replace=False)) + 1, [T]))
        first, last = bounds[0:2 * P:2], bounds[1:2 * P:2] - 1
    else:
        first = np.arange(P) + (0 if kind == "earliest" else T - P)
        last = first.copy()
    frame_tok = np.full(T, -1, np.int64)
    frame_tok[first] = np.arange(P)
    mark = np.zeros(T + 1, np.int64)                            # +1 at every first, -1 behind every last: 1 on label frames
    np.add.at(mark, first, 1)
    np.add.at(mark, last + 1, -1)
    on = np.cumsum(mark[:T]) > 0
    frame_tok = np.where(on, np.maximum.accumulate(frame_tok), -1)
    cls = np.where(on, tok[np.maximum(frame_tok, 0)], 0)
    logp = np.full((T, nc), -10.0, np.float32)
    logp[np.arange(T), cls] = 0.0
    return logp, tok.astype(np.int32), np.stack([first, last], 1).astype(np.int32), frame_tok.astype(np.int32)


@pytest.mark.parametrize("kinds", [("random", "random"), ("earliest", "random"), ("latest", "earliest")])
def test_planted_segmentation_is_found_exactly_at_the_limits(eng, kinds):
    """T = 65536, P = 16383, B = 2 (C = 4: the emission rows stay small, the lattice is the entry's largest).  The planted path has
    score 0 and every other path at most -10, so spans, frame_tok, tok_logp = 0 and score = 0 are known in closed form."""
    T, P, nc = MAX_T, MAX_P, 4
    rows = [_planted(kind, 100 + i, T, P, nc) for i, kind in enumerate(kinds)]
    logp = torch.from_numpy(np.stack([r[0] for r in rows]))
    spans, tok_logp, score, frame_tok = run(eng, logp, [T, T], np.stack([r[1] for r in rows]), [0, 0], [P, P])
    for b, (_lp, _tok, want_spans, want_ft) in enumerate(rows):
        assert score[b] == 0.0 and not tok_logp[b].any(), (kinds[b], score[b])
        assert np.array_equal(spans[b], want_spans), kinds[b]
        assert np.array_equal(frame_tok[b], want_ft), kinds[b]


# ---- isolation --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,L", [(28, 7), (300, 70)])
def test_rows_are_isolated_over_any_workspace_bytes(eng, T, L):
    """Bit for bit: a row alone, inside the ragged batch, with T padded, with NaN and garbage behind t_len, twice in a row, and over a
    workspace pre-filled with zeros and with 0xFF bytes."""
    g = torch.Generator().manual_seed(7 * T + L)
    P = L + 2
    logp = rand_logp(g, 3, T, sharp=2.0)
    tokens = torch.randint(1, NC, (3, P), generator=g).numpy().astype(np.int32)
    ts, p0, p1 = [T, max(T - 5, 0), 0], [1, 2, P], [1 + L, P, P]
    dev = eng.device
    lp_d, tok_d = logp.to(dev), torch.from_numpy(tokens).to(dev)
    n_ws = eng.lib.smtts_ctc_align_long_workspace_bytes(eng.h, 3, T + 11, P)
    snaps = []
    for fill in (0x00, 0xFF, None):                            # None: whatever the call before left behind
        if fill is not None:
            eng._workspace(n_ws).fill_(fill)
        snaps.append([o.cpu().numpy() for o in eng.ctc_align_long(lp_d, ts, tok_d, p0, p1, frames=True)])
    batch = snaps[0]
    same(batch, logp, ts, tokens, p0, p1, "batch")
    for other in snaps[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(batch, other))
    for b in (0, 1):
        eng._workspace(n_ws).fill_(0xFF)
        alone = run(eng, logp[b:b + 1], ts[b:b + 1], tokens[b:b + 1], p0[b:b + 1], p1[b:b + 1])
        assert all(a[0].tobytes() == o[b].tobytes() for a, o in zip(alone, batch)), ("alone", b)
        pad = torch.full((1, T + 11, NC), float("nan"))
        pad[0, :, ::3] = 1e30                                  # garbage and NaN behind t_len, in a row of another length
        pad[0, :ts[b]] = logp[b, :ts[b]]
        padded = run(eng, pad, ts[b:b + 1], tokens[b:b + 1], p0[b:b + 1], p1[b:b + 1])
        for a, o in zip(padded[:3], batch[:3]):
            assert a[0].tobytes() == o[b].tobytes(), ("padded", b)
        assert np.array_equal(padded[3][0, :T], batch[3][b]) and (padded[3][0, T:] == -1).all()


# ---- guard bands ------------------------------------------------------------------------------------------------------------------------
def test_the_size_query_is_the_documented_sum(eng):
    q = eng.lib.smtts_ctc_align_long_workspace_bytes
    al = lambda v: (v + 255) // 256 * 256
    for B, T, P in ((1, 1, 1), (3, 17, 5), (2, 300, 70), (1, 1030, 199), (64, 4100, 1100), (2, MAX_T, MAX_P)):
        assert q(eng.h, B, T, P) == B * (al(8 * T * ((2 * P + 1 + K - 1) // K)) + al(2 * T)), (B, T, P)
        assert q(eng.h, B, T, P) % 256 == 0
    assert q(eng.h, 1, MAX_T, MAX_P) == 512 * 2 ** 20 + 128 * 2 ** 10
    for B, T, P in ((0, 5, 5), (MAX_B + 1, 5, 5), (1, 0, 5), (1, MAX_T + 1, 5), (1, 5, 0), (1, 5, MAX_P + 1)):
        assert q(eng.h, B, T, P) == 0, (B, T, P)


@pytest.mark.parametrize("B,T,P,lens,skew", [(1, 1, 1, [1], 0), (3, 17, 5, [17, 12, 0], 4), (2, 300, 70, [300, 270], 0),
                                             (1, 1030, 199, [1030], 4)])
def test_between_guard_bands(eng, B, T, P, lens, skew):
    g = torch.Generator().manual_seed(T + P)
    a = Arena(eng.device)
    lp = a.put("logp", rand_logp(g, B, T), skew=skew)
    tl = a.put("t_len", torch.tensor(lens, dtype=torch.int32))
    tok = a.put("tokens", torch.randint(1, NC, (B, P), generator=g).to(torch.int32), skew=skew)
    p0, p1 = a.put("p0", torch.zeros(B, dtype=torch.int32)), a.put("p1", torch.full((B,), P, dtype=torch.int32))
    spans, tok_logp = a.alloc("spans", (B, P, 2), torch.int32, skew=skew), a.alloc("tok_logp", (B, P), torch.float32, skew=skew)
    frame_tok, score = a.alloc("frame_tok", (B, T), torch.int32, skew=skew), a.alloc("score", (B,), torch.float32, skew=skew)
    n_ws = eng.lib.smtts_ctc_align_long_workspace_bytes(eng.h, B, T, P)
    ws = a.workspace("ws", n_ws)                               # exactly what the query returns
    call = lambda: eng.lib.smtts_ctc_align_long(eng.h, eng._stream(), p(lp), p(tl), p(tok), p(p0), p(p1), B, T, P, NC, p(spans),
                                                p(tok_logp), p(frame_tok), p(score), p(ws), n_ws)
    ins = {n: b.view.clone() for n, b in a.bufs.items() if b.role == "in"}
    outs, snaps = ["spans", "tok_logp", "frame_tok", "score"], []
    for byte in (0x00, 0xFF):
        a.paint(byte)
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0, eng.lib.smtts_last_error(eng.h)
        a.assert_clean("smtts_ctc_align_long", f"{B}x{T}x{P} skew {skew} (guards 0x{byte:02X})")
        snaps.append({n: a[n].clone().cpu().numpy() for n in outs})
    for n in outs:
        assert snaps[0][n].tobytes() == snaps[1][n].tobytes(), n
    for n, t in ins.items():
        assert a[n].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), (n, "an input changed")
    same([snaps[0][n] for n in ("spans", "tok_logp", "score", "frame_tok")], lp.cpu().numpy(), lens, tok.cpu().numpy(), [0] * B, [P] * B, "guarded")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_name_the_entry_and_enqueue_nothing(eng):
    dev = eng.device
    B, T, P = 2, 20, 4
    lp = torch.randn(B, T, NC, device=dev).log_softmax(-1)
    tok = torch.ones(B, P, dtype=torch.int32, device=dev)
    tab = torch.tensor([[20, 12], [0, 0], [4, 4]], dtype=torch.int32, device=dev)
    spans = torch.full((B, P, 2), -7, dtype=torch.int32, device=dev)
    tok_logp, score = torch.full((B, P), -7.0, device=dev), torch.full((B,), -7.0, device=dev)
    frame_tok = torch.full((B, T), -7, dtype=torch.int32, device=dev)
    n_ws = eng.lib.smtts_ctc_align_long_workspace_bytes(eng.h, B, T, P)
    raw = torch.full((n_ws + 512,), 0x5A, dtype=torch.uint8, device=dev)
    off = (-raw.data_ptr()) % 256
    ws = raw[off:off + n_ws]

    def align(h=eng.h, lp=lp, tl=tab[0], tok=tok, p0=tab[1], p1=tab[2], B=B, T=T, P=P, Cn=NC, spans=spans, tok_logp=tok_logp,
              frame_tok=frame_tok, score=score, ws=ws, n=n_ws):
        return eng.lib.smtts_ctc_align_long(h, eng._stream(), p(lp), p(tl), p(tok), p(p0), p(p1), B, T, P, Cn, p(spans), p(tok_logp),
                                            p(frame_tok), p(score), p(ws), n)

    for kw in (dict(B=0), dict(B=MAX_B + 1), dict(T=0), dict(T=MAX_T + 1), dict(P=0), dict(P=MAX_P + 1), dict(Cn=1), dict(Cn=257),
               dict(lp=None), dict(tl=None), dict(tok=None), dict(p0=None), dict(p1=None), dict(spans=None), dict(tok_logp=None),
               dict(score=None), dict(ws=None), dict(n=n_ws - 1), dict(n=0), dict(ws=raw[off + 4:]), dict(ws=raw[off + 128:])):
        assert align(**kw) == 1 and b"smtts_ctc_align_long" in eng.lib.smtts_last_error(eng.h), kw
    assert align(h=None) == 1 and b"smtts_ctc_align_long" in eng.lib.smtts_last_error(None)
    torch.cuda.synchronize()
    assert bool((spans == -7).all()) and bool((tok_logp == -7).all()) and bool((score == -7).all()) and bool((frame_tok == -7).all())
    assert bool((raw == 0x5A).all())
    assert align() == 0 and align(frame_tok=None) == 0         # ... and the same buffers with good arguments run, with and without frame_tok
    torch.cuda.synchronize()
    assert np.isfinite(score.cpu().numpy()).all() and bool((spans >= 0).all())
    assert bool((raw[:off] == 0x5A).all()) and bool((raw[off + n_ws:] == 0x5A).all())
    # the Python face
    for bad in (lp.double(), lp[:, :, ::2], lp.cpu(), lp[0]):
        with pytest.raises(ValueError, match="ctc_align_long: logp"):
            eng.ctc_align_long(bad, [20, 12], tok, [0, 0], [4, 4])
    for bad in (tok.long(), tok[:1], tok[:, ::2], tok.cpu()):
        with pytest.raises(ValueError, match="ctc_align_long: tokens"):
            eng.ctc_align_long(lp, [20, 12], bad, [0, 0], [4, 4])
    with pytest.raises(ValueError, match="outside the supported range"):
        eng.ctc_align_long(torch.zeros(1, MAX_T + 1, 2, device=dev), [5], tok[:1], [0], [4])
    with pytest.raises(ValueError, match="outside the supported range"):
        eng.ctc_align_long(lp, [20, 12], torch.ones(B, MAX_P + 1, dtype=torch.int32, device=dev), [0, 0], [4, 4])
    with pytest.raises(ValueError, match="at most 64"):
        eng.ctc_align_long(torch.zeros(MAX_B + 1, 3, 4, device=dev), [3] * (MAX_B + 1), torch.ones(MAX_B + 1, 2, dtype=torch.int32, device=dev),
                           [0] * (MAX_B + 1), [2] * (MAX_B + 1))
    with pytest.raises(ValueError, match="one frame count"):
        eng.ctc_align_long(lp, [20], tok, [0, 0], [4, 4])
