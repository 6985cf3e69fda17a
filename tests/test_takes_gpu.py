"""GPU: takes (best-of-K sampling): the score and select kernels against the numpy restatement
(tests/helpers/takes_ref.py), bit for bit, both between guard bands, the planted defects end to end, and the Python surface on top
(synthesize_batch(takes=), synthesize_long(takes=)) against the same rows run by hand through the public call.

Every comparison here is exact: the features are integers, the total is a fixed sequence of single fp32 operations, the selection
copies rows, and a take's row in the K-fold sampler batch is the row of a by-hand batch of the same shape."""
import ctypes as C

import numpy as np
import pytest
import torch

from smalltts_amd.api import HOP_SIZE, Piece, SmallTTS, Takes, piece_seed, splice_pins, take_seed, token_groups
from smalltts_amd.weights import CodecSpec
from tests.helpers import takes_ref as T
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
F32, I32 = np.float32, np.int32
ODD = Takes(2, weights=(1.5, 2.0, 0.75, 1.25), tau_token=0.3, tau_frame=0.2)   # k plays no part in the kernels


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def same_bits(a, b):
    """The same fp32 bits; NaNs only have to sit at the same places (a NaN's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(SEED, parts=("dit", "decoder", "encoder"), codec_spec=SPEC)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def tts(eng):
    return SmallTTS(engine=eng, seed=1)


@pytest.fixture(scope="module")
def voices(tts):
    g = np.random.default_rng(0)
    return [tts.encode_voice(g.standard_normal((r, 64)).astype(np.float32)) for r in (5, 9, 7)]


# ---- the score kernel ------------------------------------------------------------------------------------------------------------------
def score_case(B, N, P, kind):
    """-> (mass (B,N,P) fp32, ns, p0, p1, takes)."""
    g = np.random.default_rng(1000 * N + P + (7 if kind == "planted" else 0))
    ns = [N] + [max(1, N - 2 * b) for b in range(1, B)]
    p0 = [0, 2, 5][:B] if (B, N, P) == (3, 7, 5) else [0] * B
    p0 = (p0 + [0] * B)[:B]
    p1 = [P] * B
    takes = Takes(2)
    if kind == "random":
        mass = g.random((B, N, P), dtype=F32)
    elif kind == "planted":
        mass = np.stack([T.planted(N, P, min(p0[b], P - 1), T.VARIANTS[b % 4]) if N >= 5 and P - p0[b] >= 4
                         else g.random((N, P), dtype=F32) for b in range(B)])
    else:   # "edges", B = 5: a random row with a NaN, a row without frames, a row without tokens, an entry exactly at each threshold
        assert B == 5 and kind == "edges"
        takes = ODD
        mass = g.random((B, N, P), dtype=F32)
        mass[0, 3, min(9, P - 1)] = np.nan
        ns[1] = 0
        p0[2] = p1[2] = 4
        mass[3:] *= F32(0.05)                             # rows 3 and 4: everything far below both thresholds ...
        mass[3, :, 5] = F32(takes.tau_token)              # ... but token 5 of row 3, exactly at tau_token wherever its span lies
        mass[4, 7, :] = F32(takes.tau_frame)              # ... and frame 7 of row 4, exactly at tau_frame (below tau_token)
        ns[3] = ns[4] = N
    return mass, ns, p0, p1, takes


def run_scores(eng, mass, ns, p0, p1, takes):
    m = torch.from_numpy(mass).to(eng.device)
    spans, score = eng.align_path(m, ns, p0, p1)
    feat, total = eng.take_scores(m, spans, score, ns, p0, p1, takes)
    return spans.cpu().numpy(), score.cpu().numpy(), feat.cpu().numpy(), total.cpu().numpy()


@pytest.mark.parametrize("B,N,P,kind", [(1, 1, 1, "random"), (3, 7, 5, "random"), (3, 7, 5, "planted"), (5, 40, 15, "random"),
                                        (5, 40, 15, "planted"), (5, 40, 15, "edges"), (2, 225, 198, "random"), (2, 225, 198, "planted")])
def test_take_scores_equals_the_restatement(eng, B, N, P, kind):
    mass, ns, p0, p1, takes = score_case(B, N, P, kind)
    spans, score, feat, total = run_scores(eng, mass, ns, p0, p1, takes)
    rfeat, rtotal = T.take_scores_ref(mass, spans, score, ns, p0, p1, takes.weights, takes.tau_token, takes.tau_frame)
    print(f"\n[take_scores {B}x{N}x{P} {kind}] feat {feat.tolist()} total {total.tolist()}")
    assert feat.dtype == I32 and np.array_equal(feat, rfeat), (feat.tolist(), rfeat.tolist())
    assert same_bits(total, rtotal), (total.tolist(), rtotal.tolist())
    again = run_scores(eng, mass, ns, p0, p1, takes)
    assert np.array_equal(again[2], feat) and same_bits(again[3], total)           # two runs: the same bits
    if (B, N, P) == (3, 7, 5):                                                      # p0 = 5 = P: a row without tokens
        assert feat[2].tolist() == [0, 0, 0, 0] and np.isposinf(total[2])
    if kind == "edges":
        assert feat[1].tolist() == [0] * 4 and feat[2].tolist() == [0] * 4 and np.isposinf(total[1:3]).all()
        assert np.isfinite(total[[0, 3, 4]]).all()
        assert feat[3, 1] == P - 1 and feat[3, 3] == 0        # token 5 alone is attended (== tau_token); every frame sees it
        assert feat[4, 1] == P and feat[4, 3] == N - 1        # frame 7 alone is not idle (== tau_frame < tau_token: all tokens skipped)


# ---- the select kernel -----------------------------------------------------------------------------------------------------------------
def select_case(G, K, N, P):
    g = np.random.default_rng(100 * G + K)
    total = g.random(G * K, dtype=F32).reshape(G, K)
    if K >= 3:
        total[0, 1] = total[0, 2] = F32(-1.0)                 # a tie for the best: the lower k
        total[-1, 0] = np.nan                                 # NaN counts as +inf
    if G >= 2 and K >= 2:
        total[1, :] = np.inf                                  # nothing finite: k = 0
        total[1, K - 1] = np.nan
    if G >= 3:
        total[2, K - 1] = -np.inf
        total[2, 0] = np.inf
    x = g.standard_normal((G * K, N, 64)).astype(F32)
    ns = [int(v) for v in g.integers(0, N + 1, G * K)]
    spans = g.integers(-1, N, (G * K, P, 2)).astype(I32)
    mass = g.random((G * K, N, P), dtype=F32)
    return total.reshape(-1), x, ns, spans, mass


@pytest.mark.parametrize("G,K,N,P", [(1, 1, 1, 1), (3, 4, 9, 5), (5, 3, 7, 6), (1, 16, 4, 3), (2, 8, 225, 198)])
def test_take_select_equals_numpy_indexing(eng, G, K, N, P):
    total, x, ns, spans, mass = select_case(G, K, N, P)
    dev = lambda a: None if a is None else torch.from_numpy(a).to(eng.device)
    for sp, ms in ((spans, mass), (None, None), (spans, None), (None, mass)):
        got = eng.take_select(dev(total), K, dev(x), ns, dev(sp), dev(ms))
        want = T.take_select_ref(total, K, x, ns, sp, ms)
        for name, a, b in zip(("x_win", "n_win", "spans_win", "mass_win", "winner"), got, want):
            assert (a is None) == (b is None), name
            if a is not None:
                a = a.cpu().numpy()
                assert a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b).astype(a.dtype).tobytes(), (name, G, K, N, P)
    win = got[4].cpu().numpy().tolist()
    if K >= 3:
        assert win[0] == 1
    if G >= 2 and K >= 2:
        assert win[1] == 0
    if G >= 3:
        assert win[2] == K - 1


# ---- both entries between guard bands ------------------------------------------------------------------------------------------------
def guarded_runs(arena, outs, call, entry, case):
    """The call with every guard painted 0x00, then 0xFF: guards clean, inputs untouched, the same output bytes both times."""
    ins = {n: b.view.clone() for n, b in arena.bufs.items() if b.role == "in"}
    snaps = []
    for byte in (0x00, 0xFF):
        arena.paint(byte)
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0, (entry, case, rc)
        arena.assert_clean(entry, f"{case} (guards 0x{byte:02X})")
        snaps.append({n: arena[n].clone() for n in outs})
    for n in outs:
        assert snaps[0][n].cpu().numpy().tobytes() == snaps[1][n].cpu().numpy().tobytes(), (entry, case, n)
    for n, t in ins.items():
        assert arena[n].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), (entry, case, n, "an input changed")
    return snaps[0]


@pytest.mark.parametrize("B,N,P,kind", [(3, 7, 5, "random"), (5, 40, 15, "edges")])
def test_take_scores_between_guard_bands(eng, B, N, P, kind):
    mass, ns, p0, p1, takes = score_case(B, N, P, kind)
    spans, score, feat, total = run_scores(eng, mass, ns, p0, p1, takes)
    a = Arena(eng.device)
    m, sp, sc = a.put("mass", torch.from_numpy(mass)), a.put("spans", torch.from_numpy(spans)), a.put("score", torch.from_numpy(score))
    tab = [a.put(n, torch.tensor(v, dtype=torch.int32)) for n, v in (("n_len", ns), ("p0", p0), ("p1", p1))]
    of, ot = a.alloc("feat", (B, 4), torch.int32), a.alloc("total", (B,), torch.float32)
    w = takes.weights
    call = lambda: eng.lib.smtts_take_scores(eng.h, eng._stream(), p(m), p(sp), p(sc), p(tab[0]), p(tab[1]), p(tab[2]), B, N, P,
                                             takes.tau_token, takes.tau_frame, w[0], w[1], w[2], w[3], p(of), p(ot))
    got = guarded_runs(a, ["feat", "total"], call, "smtts_take_scores", f"{B}x{N}x{P} {kind}")
    assert np.array_equal(got["feat"].cpu().numpy(), feat) and same_bits(got["total"].cpu().numpy(), total)


@pytest.mark.parametrize("G,K,N,P,skew", [(3, 4, 9, 5, 0), (3, 4, 9, 5, 4), (5, 3, 7, 6, 0)])
def test_take_select_between_guard_bands(eng, G, K, N, P, skew):
    """P = 5: a spans row is 40 bytes and a mass row 180, neither a multiple of 16 (the 4-byte path); skew 4: x and x_win at addresses
    that are 4-byte but not 16-byte aligned (the 4-byte path for x too); P = 6: 48-byte span rows (16-byte lanes)."""
    total, x, ns, spans, mass = select_case(G, K, N, P)
    a = Arena(eng.device)
    t, xi = a.put("total", torch.from_numpy(total)), a.put("x", torch.from_numpy(x), skew=skew)
    nl, sp, ms = a.put("n_len", torch.tensor(ns, dtype=torch.int32)), a.put("spans", torch.from_numpy(spans)), a.put("mass", torch.from_numpy(mass))
    xo = a.alloc("x_win", (G, N, 64), torch.float32, skew=skew)
    no, so = a.alloc("n_win", (G,), torch.int32), a.alloc("spans_win", (G, P, 2), torch.int32)
    mo, wo = a.alloc("mass_win", (G, N, P), torch.float32), a.alloc("winner", (G,), torch.int32)
    call = lambda: eng.lib.smtts_take_select(eng.h, eng._stream(), p(t), G, K, N, P, p(xi), p(nl), p(sp), p(ms), p(xo), p(no), p(so),
                                             p(mo), p(wo))
    names = ["x_win", "n_win", "spans_win", "mass_win", "winner"]
    got = guarded_runs(a, names, call, "smtts_take_select", f"{G}x{K}x{N}x{P} skew {skew}")
    for n, want in zip(names, T.take_select_ref(total, K, x, ns, spans, mass)):
        g_ = got[n].cpu().numpy()
        assert g_.tobytes() == np.ascontiguousarray(want).astype(g_.dtype).tobytes(), n


def test_argument_errors_name_the_entry_and_enqueue_nothing(eng):
    B, N, P, G, K = 4, 9, 5, 2, 2
    dev = eng.device
    mass, spans, score = torch.rand(B, N, P, device=dev), torch.zeros(B, P, 2, dtype=torch.int32, device=dev), torch.zeros(B, device=dev)
    tab = torch.zeros(3, B, dtype=torch.int32, device=dev)
    feat, total = torch.full((B, 4), -7, dtype=torch.int32, device=dev), torch.full((B,), -7.0, device=dev)
    x, xw = torch.rand(B, N, 64, device=dev), torch.full((G, N, 64), -7.0, device=dev)
    nw, sw = torch.full((G,), -7, dtype=torch.int32, device=dev), torch.full((G, P, 2), -7, dtype=torch.int32, device=dev)
    mw, win = torch.full((G, N, P), -7.0, device=dev), torch.full((G,), -7, dtype=torch.int32, device=dev)
    nan = float("nan")

    def scores(mass=mass, spans=spans, B=B, N=N, P=P, tt=0.1, tf=0.1, w=(1.0, 2.0, 1.0, 1.0), feat=feat, total=total):
        return eng.lib.smtts_take_scores(eng.h, eng._stream(), p(mass), p(spans), p(score), p(tab[0]), p(tab[1]), p(tab[2]), B, N, P, tt, tf,
                                         w[0], w[1], w[2], w[3], p(feat), p(total))

    def select(total=total, G=G, K=K, N=N, P=P, x=x, spans=spans, mass=mass, xw=xw, sw=sw, mw=mw, win=win):
        return eng.lib.smtts_take_select(eng.h, eng._stream(), p(total), G, K, N, P, p(x), p(tab[0]), p(spans), p(mass), p(xw), p(nw), p(sw),
                                         p(mw), p(win))

    bad_scores = [dict(B=0), dict(N=0), dict(N=226), dict(P=0), dict(P=199), dict(mass=None), dict(spans=None), dict(feat=None),
                  dict(total=None), dict(w=(-1.0, 1, 1, 1)), dict(w=(1, 1, nan, 1)), dict(tt=nan), dict(tf=nan)]
    bad_select = [dict(G=0), dict(K=0), dict(K=17), dict(N=226), dict(P=199), dict(total=None), dict(x=None), dict(xw=None), dict(win=None),
                  dict(spans=None), dict(sw=None), dict(mass=None), dict(mw=None)]
    for fn, name, cases in ((scores, b"smtts_take_scores", bad_scores), (select, b"smtts_take_select", bad_select)):
        for kw in cases:
            assert fn(**kw) == 1, (name, kw)
            assert name in eng.lib.smtts_last_error(eng.h), (name, kw)
    torch.cuda.synchronize()
    for t in (feat, total, xw, nw, sw, mw, win):
        assert bool((t == -7).all())
    assert scores() == 0 and select(total=torch.rand(B, device=dev)) == 0


# ---- planted defects, end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P,p0", [(40, 15, 0), (33, 15, 3)])
def test_the_clean_take_is_kept(eng, N, P, p0):
    order = ("stall", "skip", "clean", "idle")
    mass = torch.from_numpy(np.stack([T.planted(N, P, p0, v) for v in order])).to(eng.device)
    x = torch.randn(4, N, 64, generator=torch.Generator().manual_seed(N)).to(eng.device)
    ns, p0s, p1s = [N] * 4, [p0] * 4, [P] * 4
    spans, score = eng.align_path(mass, ns, p0s, p1s)
    feat, total = eng.take_scores(mass, spans, score, ns, p0s, p1s, Takes(4))
    x_win, n_win, spans_win, mass_win, winner = eng.take_select(total, 4, x, ns, spans, mass)
    print(f"\n[planted {N}x{P} p0 {p0}] totals {total.cpu().tolist()} feat {feat.cpu().tolist()}")
    assert winner.cpu().tolist() == [2] and n_win.cpu().tolist() == [N]
    assert torch.equal(x_win[0], x[2]) and torch.equal(spans_win[0], spans[2]) and torch.equal(mass_win[0], mass[2])
    f = feat.cpu().numpy()
    assert f[2, 1] == 0 and f[2, 3] == 0 and f[1, 1] >= 1 and f[0, 2] >= 2 * f[2, 2] and f[3, 3] == N // 5


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
TOKS = [[1, 2, 3, 4, 5, 6], [10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120], [7, 8, 9, 17, 18, 19, 27, 28, 29]]
NS = [9, 20, 14]
SEEDS = [21, 22, 23]
K = 3


@pytest.fixture(scope="module")
def by_hand(tts, eng, voices):
    """The nine sampler rows of takes=3 through the public call, and their scores by the restatement: computed once, not changed."""
    rows = [g for g in range(3) for _ in range(K)]
    audio, lat, words, raw = tts.synthesize_batch(None, [TOKS[g] for g in rows], None, frames=[NS[g] for g in rows],
                                                  voices=[voices[g] for g in rows], seeds=[take_seed(SEEDS[g], k) for g in range(3) for k in range(K)],
                                                  align=True, return_alignment=True, return_latents=True)
    feats, totals = [], []
    for r, g in enumerate(rows):
        m, sp = raw[r]
        spans, score = eng.align_path(torch.from_numpy(np.ascontiguousarray(m[None])).to(eng.device), [NS[g]], [0], [len(TOKS[g])])
        assert np.array_equal(spans.cpu().numpy()[0], sp)
        f, t = T.take_scores_ref(m[None], sp[None], score.cpu().numpy(), [NS[g]], [0], [len(TOKS[g])])
        feats.append(f[0]); totals.append(t[0])
    totals = np.asarray(totals, F32)
    return dict(audio=audio, lat=lat, words=words, raw=raw, feat=np.asarray(feats, I32).reshape(3, K, 4), total=totals.reshape(3, K),
                winner=T.winners_ref(totals, K))


def test_synthesize_batch_takes_equals_the_rows_by_hand(tts, eng, voices, by_hand):
    kw = dict(frames=NS, voices=voices, seeds=SEEDS, takes=K, return_takes=True, return_latents=True)
    rows, lat, words, raw, taken = tts.synthesize_batch(None, TOKS, None, align=True, return_alignment=True, **kw)
    win = by_hand["winner"]
    print(f"\n[takes] winners {win.tolist()} totals {by_hand['total'].tolist()}")
    assert [t[0] for t in taken] == win.tolist() and [t[1] for t in taken] == [take_seed(SEEDS[g], int(win[g])) for g in range(3)]
    pad = np.zeros((3, max(NS), 64), F32)
    for g in range(3):
        r = g * K + int(win[g])
        assert same_bits(taken[g][2], by_hand["total"][g]) and np.array_equal(taken[g][3], by_hand["feat"][g]) and taken[g][3].shape == (K, 4)
        assert lat[g].tobytes() == by_hand["lat"][r].tobytes()                       # the same sampler batch shape: exact
        assert words[g] == by_hand["words"][r]
        assert raw[g][0].tobytes() == by_hand["raw"][r][0].tobytes() and np.array_equal(raw[g][1], by_hand["raw"][r][1])
        pad[g, : NS[g]] = lat[g]
    dec = eng.codec_decode(torch.from_numpy(pad).to(eng.device)).cpu().numpy()
    for g in range(3):
        assert rows[g].shape == (1, HOP_SIZE * NS[g]) and rows[g].tobytes() == np.ascontiguousarray(dec[g, :, : HOP_SIZE * NS[g]]).tobytes()
    # without align= the words are not returned, the takes are the same, and two calls give the same bits
    a = tts.synthesize_batch(None, TOKS, None, **kw)
    b = tts.synthesize_batch(None, TOKS, None, **kw)
    assert len(a) == 3
    for g in range(3):
        assert a[0][g].tobytes() == b[0][g].tobytes() == rows[g].tobytes() and a[1][g].tobytes() == b[1][g].tobytes() == lat[g].tobytes()
        assert a[2][g][:2] == b[2][g][:2] == taken[g][:2] and same_bits(a[2][g][2], taken[g][2])
    # trim: the same winners and latents, every row a window of the untrimmed row
    cut, cut_lat, cut_taken = tts.synthesize_batch(None, TOKS, None, trim=True, **kw)
    for g in range(3):
        assert cut_lat[g].tobytes() == lat[g].tobytes() and cut_taken[g][:2] == taken[g][:2]
        n = cut[g].shape[1]
        assert 0 <= n <= rows[g].shape[1]
        if n:
            starts = [s for s in np.flatnonzero(rows[g][0] == cut[g][0, 0]) if s + n <= rows[g].shape[1]]
            assert any(np.array_equal(rows[g][0, s:s + n], cut[g][0]) for s in starts), g
    # pins on one row: every take of that row keeps them, so the winner does, bit for bit; the other rows are as before
    f0, f1 = 5, 11
    pin = splice_pins(lat[1], f0, f1)
    prow, plat, ptaken = tts.synthesize_batch(None, TOKS, None, pins=[None, pin, None], **{**kw, "seeds": [21, 220, 23]})
    assert plat[1][:f0].tobytes() == lat[1][:f0].tobytes() and plat[1][f1:].tobytes() == lat[1][f1:].tobytes()
    assert not np.array_equal(plat[1][f0:f1], lat[1][f0:f1]) and ptaken[1][1] == take_seed(220, ptaken[1][0])
    assert np.array_equal(prow[1][:, : HOP_SIZE * f0], rows[1][:, : HOP_SIZE * f0])
    for g in (0, 2):
        assert plat[g].tobytes() == lat[g].tobytes() and ptaken[g][:2] == taken[g][:2]


def test_one_take_is_the_call_without_takes(tts, eng, voices):
    kw = dict(frames=NS, voices=voices, seeds=SEEDS, return_latents=True)
    plain = tts.synthesize_batch(None, TOKS, None, **kw)
    one = tts.synthesize_batch(None, TOKS, None, takes=1, **kw)
    told = tts.synthesize_batch(None, TOKS, None, takes=1, return_takes=True, **kw)
    for g in range(3):
        assert plain[0][g].tobytes() == one[0][g].tobytes() == told[0][g].tobytes()
        assert plain[1][g].tobytes() == one[1][g].tobytes() == told[1][g].tobytes()
        k, seed, tot, ft = told[2][g]
        assert (k, seed) == (0, SEEDS[g]) and tot.shape == (1,) and ft.shape == (1, 4) and np.isfinite(tot).all()
    # without seeds= the batch draws its one seed as ever
    a = SmallTTS(engine=eng, seed=5).synthesize_batch(None, TOKS, None, frames=NS, voices=voices)
    b = SmallTTS(engine=eng, seed=5).synthesize_batch(None, TOKS, None, frames=NS, voices=voices, takes=1)
    assert all(a[g].tobytes() == b[g].tobytes() for g in range(3))
    # what the call refuses
    with pytest.raises(ValueError):
        tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, takes=2, noise=np.zeros((4, 3, 20, 64), F32))
    with pytest.raises(ValueError):
        tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, return_takes=True)
    with pytest.raises(ValueError):
        tts.synthesize_batch(None, TOKS * 7, None, frames=NS * 7, voices=voices * 7, takes=4)      # 84 sampler rows


def test_synthesize_long_takes(tts, voices):
    g = np.random.default_rng(5)
    durs = [1.3, 2.0, 0.9, 1.6]
    toks = [[int(t) for t in g.integers(1, 198, size=n)] for n in (7, 12, 5, 9)]
    kw = dict(token_lists=toks, durations=durs, seed=3, takes=2, max_batch=3)
    out, segs, words, pieces, taken = tts.synthesize_long(voices[1], return_segments=True, return_words=True, return_pieces=True,
                                                          return_takes=True, **kw)
    print(f"\n[long takes] winners {[t[0] for t in taken]}")
    assert len(pieces) == len(taken) == 4 and all(isinstance(q, Piece) for q in pieces)
    assert np.array_equal(tts.render_long(pieces, max_batch=3), out)               # the winners' latents, joined again: bit for bit
    for i, (q, (k, seed, tot, ft)) in enumerate(zip(pieces, taken)):
        assert 0 <= k < 2 and q.seed == seed == take_seed(piece_seed(3, i), k) and tot.shape == (2,) and ft.shape == (2, 4)
        assert k == int(T.winners_ref(tot, 2)[0]) and q.spans.shape == (len(toks[i]), 2)
    pos = 0
    for i, t in enumerate(toks):                                                    # a piece's words lie inside its segment
        off, n = segs[i][:2]
        for (_gi, _kind, s, e) in words[pos: pos + len(token_groups(t))]:
            assert off <= s <= e <= off + n, (i, s, e, off, n)
        pos += len(token_groups(t))
    assert pos == len(words)
    assert np.array_equal(tts.synthesize_long(voices[1], **kw), out)                # asking for less changes nothing
    # every group by hand, independent of the winner table: the group's K-fold sampler batch through the public call under the tuning
    # synthesize_long runs its batches at; piece i is the row of the take its Piece names, and that take has the lowest total
    ns = [max(1, int(d * 7.5)) for d in durs]
    prev = tts.engine.set_tuning("throughput")
    try:
        for grp in ([0, 1, 2], [3]):
            rows = [i for i in grp for _ in range(2)]
            _a, hand = tts.synthesize_batch(None, [toks[i] for i in rows], None, frames=[ns[i] for i in rows], voices=[voices[1]] * len(rows),
                                            seeds=[take_seed(piece_seed(3, i), k) for i in grp for k in range(2)], return_latents=True)
            for r, i in enumerate(grp):
                k = taken[i][0]
                assert pieces[i].latents.tobytes() == hand[2 * r + k].tobytes(), i
                assert pieces[i].latents.tobytes() != hand[2 * r + 1 - k].tobytes(), i
    finally:
        tts.engine.set_tuning(prev)


def test_synthesize_long_one_take_reports_itself(tts, voices):
    g = np.random.default_rng(6)
    durs = [1.1, 1.9, 0.8]
    toks = [[int(t) for t in g.integers(1, 198, size=n)] for n in (6, 11, 5)]
    kw = dict(token_lists=toks, durations=durs, seed=4, max_batch=2)
    plain = tts.synthesize_long(voices[0], **kw)
    assert np.array_equal(tts.synthesize_long(voices[0], takes=1, **kw), plain)
    out, pieces, taken = tts.synthesize_long(voices[0], takes=1, return_takes=True, return_pieces=True, **kw)
    assert np.array_equal(out, plain) and len(taken) == 3
    for i, (k, seed, tot, ft) in enumerate(taken):
        assert (k, seed) == (0, piece_seed(4, i)) and pieces[i].seed == seed
        assert tot.shape == (1,) and ft.shape == (1, 4) and np.isfinite(tot).all() and ft[0, 0] >= ns_of(durs[i])


def ns_of(d):
    return max(1, int(d * 7.5))


def test_respeak_takes(tts, voices):
    toks, n, (f0, f1) = TOKS[1], 20, (5, 11)
    (orig,), (lat,) = tts.synthesize_batch(None, [toks], None, frames=[n], voices=[voices[1]], seeds=[6], return_latents=True)
    audio, new, taken = tts.respeak(toks, lat, (f0, f1), voice=voices[1], seed=60, takes=K, return_takes=True, prefix_len=2)
    k, seed, tot, ft = taken
    assert seed == take_seed(60, k) and tot.shape == (K,) and ft.shape == (K, 4) and k == int(T.winners_ref(tot, K)[0])
    assert (ft[:, 1] <= len(toks) - 2).all()                                        # the prefix is left out of the score
    assert new[:f0].tobytes() == lat[:f0].tobytes() and new[f1:].tobytes() == lat[f1:].tobytes()          # every take keeps the pins
    assert np.array_equal(audio[:, : HOP_SIZE * f0], orig[:, : HOP_SIZE * f0])
    # the same three rows by hand: the winner is row k of them
    hand = tts.synthesize_batch(None, [toks] * K, None, frames=[n] * K, voices=[voices[1]] * K, seeds=[take_seed(60, j) for j in range(K)],
                                return_latents=True, pins=[splice_pins(lat, f0, f1)] * K)
    assert hand[1][k].tobytes() == new.tobytes()
