"""GPU: repair (re-speak only the badly aligned words of a take): the plan and keep kernels against the numpy restatement
(tests/helpers/repair_ref.py), exactly, both between guard bands, and the Python surface on top (synthesize_batch(repair=),
synthesize_long(repair=)) against the same passes run by hand through the public calls.

Every comparison here is exact: the plan is integers decided by single fp32 comparisons, the keep rule copies rows, and a repair pass
is the pinned sampler on a batch of the same shape as the by-hand call."""
import ctypes as C

import numpy as np
import pytest
import torch

from smalltts_amd.api import HOP_SIZE, Piece, Repair, SmallTTS, Takes, repair_seed
from smalltts_amd.weights import CodecSpec
from tests.helpers import repair_ref as R
from tests.helpers import takes_ref as T
from tests.helpers.align_ref import dp_align
from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
F32, I32 = np.float32, np.int32


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


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


# ---- the plan kernel -------------------------------------------------------------------------------------------------------------------
def random_spans(g, N, P, n, p0, p1):
    """A monotone cover of frames [0, n) by the tokens [p0, p1), (-1, -1) elsewhere; every seventh token gets a span the entry has to
    survive instead: empty, reversed, or running past the row."""
    sp = np.full((P, 2), -1, I32)
    Pw = p1 - p0
    if n <= 0 or Pw <= 0:
        return sp
    cuts = np.sort(g.integers(0, n, Pw - 1)) if Pw > 1 else np.zeros(0, np.int64)
    first = np.concatenate([[0], cuts]).astype(I32)
    last = np.concatenate([cuts, [n - 1]]).astype(I32)
    sp[p0:p1, 0], sp[p0:p1, 1] = first, last
    for i, t in enumerate(range(p0 + 3, p1, 7)):
        sp[t] = [(-1, -1), (int(sp[t, 1]) + 1, int(sp[t, 0])), (int(sp[t, 0]), 10 ** 6)][i % 3]
    return sp


def plan_case(eng, B, N, P, kind):
    """-> (mass (B,N,P) fp32, spans (B,P,2) int32, ns, p0, p1, tau)."""
    g = np.random.default_rng(2000 * N + P + {"random": 0, "planted": 7, "edges": 13}[kind])
    ns = [N] + [max(1, N - 2 * b) for b in range(1, B)]
    p0 = ([0, 2, 5] if (B, N, P) == (3, 7, 5) else [0] * B)[:B]
    p1 = [P] * B
    tau = 0.1
    if kind == "random":
        tau = 0.9                                             # uniform mass: a span of L frames attends with probability 1 - 0.9^L
        mass = g.random((B, N, P), dtype=F32)
        spans = np.stack([random_spans(g, N, P, ns[b], p0[b], p1[b]) for b in range(B)])
        return mass, spans, ns, p0, p1, tau
    if kind == "planted":
        mass = np.stack([T.planted(N, P, min(p0[b], P - 1), T.VARIANTS[(b + 1) % 4]) if N >= 5 and P - p0[b] >= 4
                         else g.random((N, P), dtype=F32) for b in range(B)])
    else:   # "edges", B = 5: a NaN in a span, a row without frames, a row without tokens, one entry exactly at the threshold
        assert B == 5
        tau = 0.3
        mass = g.random((B, N, P), dtype=F32)
        mass[0, :, min(9, P - 1)] = np.nan                   # token 9 of row 0: a span of NaNs never attends
        ns[1] = 0
        p0[2] = p1[2] = 4
        mass[3:] *= F32(0.05)                                 # rows 3 and 4: everything far below the threshold ...
        mass[3, :, 5] = F32(tau)                              # ... but token 5 of row 3, exactly at it wherever its span lies
        ns[3] = ns[4] = N
    m = torch.from_numpy(mass).to(eng.device)
    spans = eng.align_path(m, ns, p0, p1)[0].cpu().numpy()
    return mass, spans, ns, p0, p1, tau


SETTINGS = [(8, 2), (1, 0), (225, 32), (3, 32), (225, 0)]     # (max_span, margin): the defaults and both ends of both ranges


@pytest.mark.parametrize("B,N,P,kind", [(1, 1, 1, "random"), (3, 7, 5, "random"), (3, 7, 5, "planted"), (5, 40, 15, "random"),
                                        (5, 40, 15, "planted"), (5, 40, 15, "edges"), (2, 225, 198, "random"), (2, 225, 198, "planted")])
def test_repair_plan_equals_the_restatement(eng, B, N, P, kind):
    mass, spans, ns, p0, p1, tau = plan_case(eng, B, N, P, kind)
    g = np.random.default_rng(B * N)
    keep = g.random((B, N)) < 0.3
    m, sp = torch.from_numpy(mass).to(eng.device), torch.from_numpy(spans).to(eng.device)
    seen = set()
    for max_span, margin in SETTINGS:
        for kp in (None, keep):
            rp = Repair(1, tau_token=tau, max_span=max_span, margin=margin)
            kd = None if kp is None else torch.from_numpy(kp).to(eng.device)
            pin, counts = eng.repair_plan(m, sp, ns, p0, p1, rp, kd)
            pin2, counts2 = eng.repair_plan(m, sp, ns, p0, p1, rp, kd)
            rpin, rcounts = R.repair_plan_ref(mass, spans, ns, p0, p1, kp, tau, max_span, margin)
            assert pin.dtype == torch.bool and counts.dtype == torch.int32
            got, gc = pin.view(torch.uint8).cpu().numpy(), counts.cpu().numpy()
            assert np.array_equal(gc, rcounts), (max_span, margin, kp is not None, gc.tolist(), rcounts.tolist())
            assert np.array_equal(got, rpin), (max_span, margin, kp is not None)
            assert torch.equal(pin2.view(torch.uint8), pin.view(torch.uint8)) and torch.equal(counts2, counts)   # two runs: the same bits
            seen.add(tuple(gc[:, 1].tolist()))
            if kp is None and (max_span, margin) == (8, 2):
                print(f"\n[repair_plan {B}x{N}x{P} {kind}] counts {gc.tolist()}")
                if (B, N, P) == (3, 7, 5):                    # p0 = 5 = P: a row without tokens
                    assert gc[2].tolist() == [0, 0] and not got[2].any()
                if kind == "planted" and (N, P) == (40, 15):  # row 0: the skip of the CPU test's table
                    assert gc[0].tolist() == [1, 5]
            if kp is None and (max_span, margin) == (225, 0) and kind == "edges":   # no span is too long: the threshold alone decides
                assert gc[1].tolist() == [0, 0] and gc[2].tolist() == [0, 0] and not got[1].any() and not got[2].any()
                assert gc[0, 0] >= 1                          # the NaN token
                assert gc[3, 0] == P - 1 and gc[4, 0] == P    # token 5 of row 3 alone attends (== tau)
    if N > 1:
        assert len(seen) > 1                                  # the settings matter at this shape


# ---- the keep kernel -------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
RULE = [(2.0, 1.0, 3), (2.0, 1.0, 0), (1.0, 1.0, 2), (NAN, INF, 1), (INF, 7.0, 1), (NAN, 5.0, 1), (1.0, NAN, 4)]   # (cur, new, freed frames)
WANT = [1, 0, 0, 0, 1, 1, 0]          # lower: kept; nothing freed: never; a tie: no; NaN counts as +inf; +inf loses to anything finite


def keep_case(G, N, P):
    g = np.random.default_rng(100 * G + N)
    rows = [(4 if G == 3 else 0) + i for i in range(G)]
    rule = [RULE[r % len(RULE)] for r in rows]
    cur, new = np.asarray([r[0] for r in rule], F32), np.asarray([r[1] for r in rule], F32)
    counts = np.asarray([[1, r[2]] for r in rule], I32)
    d = dict(total_cur=cur, total_new=new, counts=counts,
             feat_cur=g.integers(0, 50, (G, 4)).astype(I32), feat_new=g.integers(50, 99, (G, 4)).astype(I32),
             x_cur=g.standard_normal((G, N, 64)).astype(F32), x_new=g.standard_normal((G, N, 64)).astype(F32),
             spans_cur=g.integers(-1, N, (G, P, 2)).astype(I32), spans_new=g.integers(-1, N, (G, P, 2)).astype(I32),
             mass_cur=g.random((G, N, P), dtype=F32), mass_new=g.random((G, N, P), dtype=F32))
    return d, [WANT[r % len(RULE)] for r in rows]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("G,N,P", [(1, 1, 1), (3, 9, 5), (5, 7, 6), (2, 225, 198)])
def test_repair_keep_equals_numpy(eng, G, N, P):
    d, want = keep_case(G, N, P)
    for with_spans, with_mass in ((True, True), (False, False), (True, False), (False, True)):
        dev = {k: torch.from_numpy(v.copy()).to(eng.device) for k, v in d.items()}
        sc, sn = (dev["spans_cur"], dev["spans_new"]) if with_spans else (None, None)
        mc, mn = (dev["mass_cur"], dev["mass_new"]) if with_mass else (None, None)
        t, f, kept = eng.repair_keep(dev["total_cur"], dev["total_new"], dev["counts"], dev["feat_cur"], dev["feat_new"], dev["x_cur"],
                                     dev["x_new"], sc, sn, mc, mn)
        rt, rf, rk, rx, rs, rm = R.repair_keep_ref(*(d[k] for k in ("total_cur", "total_new", "counts", "feat_cur", "feat_new", "x_cur",
                                                                    "x_new", "spans_cur", "spans_new", "mass_cur", "mass_new")))
        assert kept.cpu().numpy().tolist() == rk.tolist() == want, (G, kept.cpu().tolist(), want)
        assert same(t.cpu().numpy(), rt) and same(f.cpu().numpy(), rf)           # (the bits of a NaN total too: it is copied, not computed)
        assert same(dev["x_cur"].cpu().numpy(), rx)
        assert same(dev["spans_cur"].cpu().numpy(), rs if with_spans else d["spans_cur"])     # a NULL pair is left alone
        assert same(dev["mass_cur"].cpu().numpy(), rm if with_mass else d["mass_cur"])
        for k in ("total_cur", "total_new", "counts", "feat_cur", "feat_new", "x_new", "spans_new", "mass_new"):
            assert same(dev[k].cpu().numpy(), d[k]), k                           # the inputs are only read
        for g_ in range(G):                                                       # a row that is not replaced keeps its bits
            if not want[g_]:
                assert same(dev["x_cur"][g_].cpu().numpy(), d["x_cur"][g_]) and same(dev["mass_cur"][g_].cpu().numpy(), d["mass_cur"][g_])


# ---- both entries between guard bands ------------------------------------------------------------------------------------------------
def guarded_runs(arena, outs, call, entry, case, inplace=()):
    """The call with every guard painted 0x00, then 0xFF: guards clean, inputs untouched, the same output bytes both times.  `inplace`:
    inputs the entry is meant to change; they are set back before every run and compared like outputs."""
    ins = {n: b.view.clone() for n, b in arena.bufs.items() if b.role == "in"}
    snaps = []
    for byte in (0x00, 0xFF):
        arena.paint(byte)
        for n in inplace:
            arena[n].copy_(ins[n])
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0, (entry, case, rc)
        arena.assert_clean(entry, f"{case} (guards 0x{byte:02X})")
        snaps.append({n: arena[n].clone() for n in list(outs) + list(inplace)})
    for n in snaps[0]:
        assert snaps[0][n].cpu().numpy().tobytes() == snaps[1][n].cpu().numpy().tobytes(), (entry, case, n)
    for n, t in ins.items():
        if n not in inplace:
            assert arena[n].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), (entry, case, n, "an input changed")
    return snaps[0]


@pytest.mark.parametrize("B,N,P,kind,with_keep", [(3, 7, 5, "random", True), (3, 7, 5, "random", False), (5, 40, 15, "edges", True)])
def test_repair_plan_between_guard_bands(eng, B, N, P, kind, with_keep):
    """N = 7: a pin row is 7 bytes, rows at odd addresses; the guards right behind the last row's last byte."""
    mass, spans, ns, p0, p1, tau = plan_case(eng, B, N, P, kind)
    keep = (np.random.default_rng(5).random((B, N)) < 0.3) if with_keep else None
    a = Arena(eng.device)
    m, sp = a.put("mass", torch.from_numpy(mass)), a.put("spans", torch.from_numpy(spans))
    tab = [a.put(n, torch.tensor(v, dtype=torch.int32)) for n, v in (("n_len", ns), ("p0", p0), ("p1", p1))]
    kp = a.put("keep", torch.from_numpy(keep)) if with_keep else None
    op, oc = a.alloc("pin", (B, N), torch.uint8), a.alloc("counts", (B, 2), torch.int32)
    call = lambda: eng.lib.smtts_repair_plan(eng.h, eng._stream(), p(m), p(sp), p(tab[0]), p(tab[1]), p(tab[2]), p(kp), B, N, P, tau, 8, 32,
                                             p(op), p(oc))
    got = guarded_runs(a, ["pin", "counts"], call, "smtts_repair_plan", f"{B}x{N}x{P} {kind} keep {with_keep}")
    rpin, rcounts = R.repair_plan_ref(mass, spans, ns, p0, p1, keep, tau, 8, 32)
    assert np.array_equal(got["pin"].cpu().numpy(), rpin) and np.array_equal(got["counts"].cpu().numpy(), rcounts)


@pytest.mark.parametrize("G,N,P,skew", [(3, 9, 5, 0), (3, 9, 5, 4), (5, 7, 6, 0)])
def test_repair_keep_between_guard_bands(eng, G, N, P, skew):
    """P = 5: a spans row is 40 bytes and a mass row 180, neither a multiple of 16 (the 4-byte path); skew 4: x_cur and x_new at
    addresses that are 4-byte but not 16-byte aligned (the 4-byte path for x too); P = 6: 48-byte span rows (16-byte lanes)."""
    d, want = keep_case(G, N, P)
    a = Arena(eng.device)
    v = {k: a.put(k, torch.from_numpy(t), skew=skew if k in ("x_cur", "x_new") else 0) for k, t in d.items()}
    ot, of, ok = a.alloc("total_out", (G,), torch.float32), a.alloc("feat_out", (G, 4), torch.int32), a.alloc("kept", (G,), torch.int32)
    call = lambda: eng.lib.smtts_repair_keep(eng.h, eng._stream(), G, N, P, p(v["total_cur"]), p(v["total_new"]), p(v["counts"]),
                                             p(v["feat_cur"]), p(v["feat_new"]), p(v["x_cur"]), p(v["x_new"]), p(v["spans_cur"]),
                                             p(v["spans_new"]), p(v["mass_cur"]), p(v["mass_new"]), p(ot), p(of), p(ok))
    got = guarded_runs(a, ["total_out", "feat_out", "kept"], call, "smtts_repair_keep", f"{G}x{N}x{P} skew {skew}",
                       inplace=("x_cur", "spans_cur", "mass_cur"))
    ref = R.repair_keep_ref(*(d[k] for k in ("total_cur", "total_new", "counts", "feat_cur", "feat_new", "x_cur", "x_new", "spans_cur",
                                             "spans_new", "mass_cur", "mass_new")))
    for n, r in zip(("total_out", "feat_out", "kept", "x_cur", "spans_cur", "mass_cur"), ref):
        assert same(got[n].cpu().numpy(), r), n
    assert got["kept"].cpu().tolist() == want


def test_argument_errors_name_the_entry_and_enqueue_nothing(eng):
    B, N, P = 4, 9, 5
    dev = eng.device
    mass, spans = torch.rand(B, N, P, device=dev), torch.zeros(B, P, 2, dtype=torch.int32, device=dev)
    tab = torch.zeros(3, B, dtype=torch.int32, device=dev)
    tab[0] = N
    tab[2] = P
    pin, counts = torch.full((B, N), 7, dtype=torch.uint8, device=dev), torch.full((B, 2), -7, dtype=torch.int32, device=dev)
    tc, tn = torch.ones(B, device=dev), torch.zeros(B, device=dev)              # every row would be replaced
    cn = torch.ones(B, 2, dtype=torch.int32, device=dev)
    fc, fn = torch.zeros(B, 4, dtype=torch.int32, device=dev), torch.ones(B, 4, dtype=torch.int32, device=dev)
    xc, xn = torch.full((B, N, 64), -7.0, device=dev), torch.rand(B, N, 64, device=dev)
    sc, sn = torch.full((B, P, 2), -7, dtype=torch.int32, device=dev), torch.ones(B, P, 2, dtype=torch.int32, device=dev)
    mc, mn = torch.full((B, N, P), -7.0, device=dev), torch.rand(B, N, P, device=dev)
    to, fo, ko = torch.full((B,), -7.0, device=dev), torch.full((B, 4), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)
    nan = float("nan")

    def plan(mass=mass, spans=spans, n_len=tab[0], p0=tab[1], p1=tab[2], B=B, N=N, P=P, tau=0.1, span=8, margin=2, pin=pin, counts=counts):
        return eng.lib.smtts_repair_plan(eng.h, eng._stream(), p(mass), p(spans), p(n_len), p(p0), p(p1), None, B, N, P, tau, span, margin,
                                         p(pin), p(counts))

    def keep(G=B, N=N, P=P, tc=tc, tn=tn, cn=cn, fc=fc, fn=fn, xc=xc, xn=xn, sc=sc, sn=sn, mc=mc, mn=mn, to=to, fo=fo, ko=ko):
        return eng.lib.smtts_repair_keep(eng.h, eng._stream(), G, N, P, p(tc), p(tn), p(cn), p(fc), p(fn), p(xc), p(xn), p(sc), p(sn), p(mc),
                                         p(mn), p(to), p(fo), p(ko))

    bad_plan = [dict(B=0), dict(B=65537), dict(N=0), dict(N=226), dict(P=0), dict(P=199), dict(mass=None), dict(spans=None), dict(n_len=None),
                dict(p0=None), dict(p1=None), dict(pin=None), dict(counts=None), dict(tau=nan), dict(span=0), dict(span=226),
                dict(margin=-1), dict(margin=33)]
    bad_keep = [dict(G=0), dict(G=65536), dict(N=0), dict(N=226), dict(P=0), dict(P=199), dict(tc=None), dict(tn=None), dict(cn=None),
                dict(fc=None), dict(fn=None), dict(xc=None), dict(xn=None), dict(to=None), dict(fo=None), dict(ko=None), dict(sc=None),
                dict(sn=None), dict(mc=None), dict(mn=None)]
    for fn_, name, cases in ((plan, b"smtts_repair_plan", bad_plan), (keep, b"smtts_repair_keep", bad_keep)):
        for kw in cases:
            assert fn_(**kw) == 1, (name, kw)
            assert name in eng.lib.smtts_last_error(eng.h), (name, kw)
    assert eng.lib.smtts_repair_plan(None, eng._stream(), p(mass), p(spans), p(tab[0]), p(tab[1]), p(tab[2]), None, B, N, P, 0.1, 8, 2,
                                     p(pin), p(counts)) == 1
    assert b"smtts_repair_plan" in eng.lib.smtts_last_error(None)
    torch.cuda.synchronize()
    assert bool((pin == 7).all())
    for t in (counts, xc, sc, mc, to, fo, ko):
        assert bool((t == -7).all())
    assert plan() == 0 and keep() == 0
    torch.cuda.synchronize()
    assert ko.cpu().tolist() == [1] * B and torch.equal(xc, xn) and torch.equal(sc, sn) and torch.equal(mc, mn)
    # the wrappers refuse what the entries would, as ValueError
    with pytest.raises(ValueError):
        eng.repair_plan(mass.double(), spans, [N] * B, [0] * B, [P] * B, Repair())
    with pytest.raises(ValueError):
        eng.repair_plan(mass, spans, [N] * B, [0] * B, [P] * B, Repair(), keep=torch.zeros(B, N + 1, dtype=torch.bool, device=dev))
    with pytest.raises(ValueError):
        eng.repair_keep(tc, tn, cn, fc, fn, xc, xn, sc, None)
    with pytest.raises(ValueError):
        eng.repair_keep(tc, tn, cn, fc, fn, xc, xn[:, :-1].contiguous())


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------
TOKS = [[1, 2, 3, 4, 5, 6], [10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120], [7, 8, 9, 17, 18, 19, 27, 28, 29]]
NS = [9, 20, 14]
SEEDS = [21, 22, 23]
AL = dict(align=True, return_alignment=True, return_latents=True)


def padded(raw, ns, toks):
    """Per-row (mass (n, P_b), spans (P_b, 2)) -> the batch's (G, Nmax, Pmax) mass and (G, Pmax, 2) spans, zeros / (-1, -1) behind."""
    G, Nm, Pm = len(raw), max(ns), max(len(t) for t in toks)
    mass, spans = np.zeros((G, Nm, Pm), F32), np.full((G, Pm, 2), -1, I32)
    for g, (m, sp) in enumerate(raw):
        mass[g, : m.shape[0], : m.shape[1]] = m
        spans[g, : sp.shape[0]] = sp
    return mass, spans


def totals_of(raw, ns, toks, takes=None):
    """The rows' totals from the host restatements alone: dp_align for the path and its cost, take_scores_ref for the total."""
    out = []
    for g, (m, sp) in enumerate(raw):
        spans, score, _path = dp_align(m, ns[g], 0, len(toks[g]))
        assert np.array_equal(spans, sp)
        kw = {} if takes is None else dict(weights=takes.weights, tau_token=takes.tau_token, tau_frame=takes.tau_frame)
        out.append(T.take_scores_ref(m[None], spans[None], [score], [ns[g]], [0], [len(toks[g])], **kw)[1][0])
    return np.asarray(out, F32)


def span_peaks(raw):
    return np.asarray([m[sp[t, 0]: sp[t, 1] + 1, t].max() for m, sp in raw for t in range(sp.shape[0]) if sp[t, 0] >= 0], F32)


def one_round_by_hand(tts, toks, ns, voices, base, seeds, rp, pins=None, takes=None):
    """One repair round on the rows `base` = (audio rows, latents, words, raw alignment) through the public call: the plan by the
    restatement, the pinned call, the scores, the keep rule.  -> (merged (rows, latents, words, raw), report pieces, plan, replace)."""
    rows0, x0, words0, raw0 = base
    mass, spans = padded(raw0, ns, toks)
    keep = None
    if pins is not None:
        keep = np.zeros(mass.shape[:2], bool)
        for g, pn in enumerate(pins):
            if pn is not None:
                keep[g, : ns[g]] = pn[1]
    plan, counts = R.repair_plan_ref(mass, spans, ns, [0] * len(ns), [len(t) for t in toks], keep, rp.tau_token, rp.max_span, rp.margin)
    rows1, x1, words1, raw1 = tts.synthesize_batch(None, toks, None, frames=ns, voices=voices, seeds=[repair_seed(s, 1) for s in seeds],
                                                   pins=[(x0[g], plan[g, : ns[g]].astype(bool)) for g in range(len(ns))], **AL)
    t0, t1 = totals_of(raw0, ns, toks, takes), totals_of(raw1, ns, toks, takes)
    rep = R.replace_ref(t0, t1, counts)
    pick = lambda a, b: [b[g] if rep[g] else a[g] for g in range(len(ns))]
    merged = (pick(rows0, rows1), pick(x0, x1), pick(words0, words1), pick(raw0, raw1))
    return merged, (rep.astype(I32), counts, t0, np.where(rep, t1, t0).astype(F32)), plan, rep


def assert_rows_equal(got, want, what):
    rows, lat, words, raw = got
    wrows, wlat, wwords, wraw = want
    for g in range(len(wlat)):
        assert lat[g].tobytes() == wlat[g].tobytes(), (what, g, "latents")
        assert rows[g].shape == wrows[g].shape and rows[g].tobytes() == np.ascontiguousarray(wrows[g]).tobytes(), (what, g, "audio")
        assert words[g] == wwords[g], (what, g, "words")
        assert raw[g][0].tobytes() == wraw[g][0].tobytes() and np.array_equal(raw[g][1], wraw[g][1]), (what, g, "alignment")


def assert_report(got, want, what):
    kept, counts, before, after = want
    for g, (k, c, b, a) in enumerate(got):
        assert k.shape == (1,) and c.shape == (1, 2) and b.shape == (1,) and a.shape == (1,) and b.dtype == a.dtype == F32
        assert int(k[0]) == int(kept[g]) and c[0].tolist() == counts[g].tolist(), (what, g, k, c, kept, counts)
        assert b.tobytes() == before[g: g + 1].tobytes() and a.tobytes() == after[g: g + 1].tobytes(), (what, g, b, a, before, after)


@pytest.fixture(scope="module")
def plain(tts, voices):
    """The three rows without repair through the public call, and the threshold that makes about half of their tokens bad: the median
    of the tokens' span peaks.  Computed once, not changed."""
    base = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=SEEDS, **AL)
    return dict(base=base, tau=float(F32(np.median(span_peaks(base[3])))))


def test_synthesize_batch_repair_equals_the_passes_by_hand(tts, eng, voices, plain):
    rp = Repair(1, tau_token=plain["tau"], max_span=225, margin=0)
    want, report, plan, rep = one_round_by_hand(tts, TOKS, NS, voices, plain["base"], SEEDS, rp)
    free = [int(NS[g] - plan[g, : NS[g]].sum()) for g in range(3)]
    print(f"\n[repair] tau {rp.tau_token:.6f} (bad, free) {report[1].tolist()} of {NS} frames, totals {report[2].tolist()} -> "
          f"{report[3].tolist()}, replaced {rep.tolist()}")
    assert any(0 < free[g] < NS[g] for g in range(3)), free      # a partial plan, or this test shows nothing
    kw = dict(frames=NS, voices=voices, seeds=SEEDS, repair=rp, return_repair=True)
    got = tts.synthesize_batch(None, TOKS, None, **AL, **kw)
    assert len(got) == 5
    assert_rows_equal(got[:4], want, "repair")
    assert_report(got[4], report, "repair")
    x0 = plain["base"][1]
    for g in range(3):
        pinned = plan[g, : NS[g]].astype(bool)
        if rep[g]:                                               # what the plan pinned is the first pass's, bit for bit
            assert got[1][g][pinned].tobytes() == x0[g][pinned].tobytes() and not np.array_equal(got[1][g][~pinned], x0[g][~pinned])
        else:
            assert got[1][g].tobytes() == x0[g].tobytes()
    # the audio is the decode of the merged latents
    pad = np.zeros((3, max(NS), 64), F32)
    for g in range(3):
        pad[g, : NS[g]] = got[1][g]
    dec = eng.codec_decode(torch.from_numpy(pad).to(eng.device)).cpu().numpy()
    for g in range(3):
        assert got[0][g].tobytes() == np.ascontiguousarray(dec[g, :, : HOP_SIZE * NS[g]]).tobytes()
    # without align= no words come back, the repair is the same, and two calls give the same bits
    a = tts.synthesize_batch(None, TOKS, None, return_latents=True, **kw)
    b = tts.synthesize_batch(None, TOKS, None, return_latents=True, **kw)
    assert len(a) == 3
    for g in range(3):
        assert a[0][g].tobytes() == b[0][g].tobytes() == got[0][g].tobytes() and a[1][g].tobytes() == b[1][g].tobytes() == got[1][g].tobytes()
    assert_report(a[2], report, "repair without align")
    # trim: the same latents, every row a window of the untrimmed row
    cut, cut_lat, _rep = tts.synthesize_batch(None, TOKS, None, return_latents=True, trim=True, **kw)
    for g in range(3):
        assert cut_lat[g].tobytes() == got[1][g].tobytes()
        n = cut[g].shape[1]
        assert 0 <= n <= got[0][g].shape[1]
        if n:
            starts = [s for s in np.flatnonzero(got[0][g][0] == cut[g][0, 0]) if s + n <= got[0][g].shape[1]]
            assert any(np.array_equal(got[0][g][0, s:s + n], cut[g][0]) for s in starts), g


def test_a_row_with_nothing_bad_comes_back_as_it_was(tts, voices, plain):
    got = tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, seeds=SEEDS, repair=Repair(1, tau_token=0.0, max_span=225, margin=0),
                               return_repair=True, **AL)
    assert_rows_equal(got[:4], plain["base"], "nothing bad")
    for kept, counts, before, after in got[4]:
        assert kept.tolist() == [0] and counts.tolist() == [[0, 0]] and before.tobytes() == after.tobytes()


def test_repair_launches(tts, eng, voices, plain):
    kw = dict(frames=NS, voices=voices, seeds=SEEDS)
    launches = lambda rep: {e["name"]: e["launches"] for e in rep if "repair" in e["name"]}
    eng.profile(True)
    try:
        tts.synthesize_batch(None, TOKS, None, **kw)
        tts.synthesize_batch(None, TOKS, None, takes=2, align=True, **kw)
        torch.cuda.synchronize()
        off = eng.profile_report()
        tts.synthesize_batch(None, TOKS, None, repair=Repair(2, tau_token=plain["tau"]), **kw)
        torch.cuda.synchronize()
        on = eng.profile_report()
    finally:
        eng.profile(False)
    assert launches(off) == {} and len(off) > 0                  # without repair= not one launch of it
    assert launches(on) == {"repair_plan": 2, "repair_keep": 2}, launches(on)


def test_what_the_calls_refuse(tts, voices):
    kw = dict(frames=NS, voices=voices, seeds=SEEDS)
    with pytest.raises(ValueError):
        tts.synthesize_batch(None, TOKS, None, frames=NS, voices=voices, repair=1, noise=np.zeros((4, 3, 20, 64), F32))
    with pytest.raises(ValueError):
        tts.synthesize_batch(None, TOKS, None, repair=1, start_step=1, pins=[(np.zeros((n, 64), F32), np.ones(n, bool)) for n in NS], **kw)
    with pytest.raises(ValueError):
        tts.synthesize_batch(None, TOKS, None, return_repair=True, **kw)
    with pytest.raises(ValueError):
        tts.synthesize_long(voices[0], token_lists=TOKS, durations=1.0, return_repair=True)
    with pytest.raises(TypeError):
        tts.synthesize_batch(None, TOKS, None, repair=1.5, **kw)


def test_repair_behind_takes_equals_the_composition_by_hand(tts, voices, plain):
    tk = Takes(2, weights=(1.5, 2.0, 0.75, 1.25), tau_token=0.3, tau_frame=0.2)
    rp = Repair(1, tau_token=plain["tau"], max_span=225, margin=0)
    kw = dict(frames=NS, voices=voices, seeds=SEEDS, takes=tk, return_takes=True)
    win = tts.synthesize_batch(None, TOKS, None, **AL, **kw)                      # the winners: the rows repair starts from
    want, report, plan, rep = one_round_by_hand(tts, TOKS, NS, voices, win[:4], SEEDS, rp, takes=tk)
    got = tts.synthesize_batch(None, TOKS, None, repair=rp, return_repair=True, **AL, **kw)
    print(f"\n[takes + repair] winners {[t[0] for t in win[4]]} (bad, free) {report[1].tolist()} replaced {rep.tolist()}")
    assert len(got) == 6
    assert_rows_equal(got[:4], want, "takes + repair")
    assert_report(got[5], report, "takes + repair")
    for g in range(3):                                                            # the takes' report is that of the call without repair
        assert got[4][g][:2] == win[4][g][:2] and got[4][g][2].tobytes() == win[4][g][2].tobytes() and np.array_equal(got[4][g][3], win[4][g][3])
        assert got[5][g][2].tobytes() == win[4][g][2][win[4][g][0]: win[4][g][0] + 1].tobytes()   # repair starts from the winner's total


def test_the_callers_pins_stay_pinned(tts, voices, plain):
    rp = Repair(1, tau_token=plain["tau"], max_span=225, margin=0)
    x0 = plain["base"][1]
    g = np.random.default_rng(3)
    pins = [None, (x0[1], g.random(NS[1]) < 0.5), (x0[2], np.ones(NS[2], bool))]  # row 2: everything kept, nothing to repair
    kw = dict(frames=NS, voices=voices, seeds=[31, 32, 33], pins=pins)
    base = tts.synthesize_batch(None, TOKS, None, **AL, **kw)
    want, report, plan, rep = one_round_by_hand(tts, TOKS, NS, voices, base, [31, 32, 33], rp, pins=pins)
    got = tts.synthesize_batch(None, TOKS, None, repair=rp, return_repair=True, **AL, **kw)
    print(f"\n[pins + repair] (bad, free) {report[1].tolist()} replaced {rep.tolist()}")
    assert_rows_equal(got[:4], want, "pins + repair")
    assert_report(got[4], report, "pins + repair")
    for r in (1, 2):
        keep = pins[r][1]
        assert got[1][r][keep].tobytes() == x0[r][keep].tobytes()                 # the caller's bits
        assert (plan[r, : NS[r]][keep] == 1).all()                                # the plan never frees a kept frame
    assert report[1][2, 1] == 0 and int(got[4][2][0][0]) == 0 and got[1][2].tobytes() == x0[2].tobytes()


def test_synthesize_long_repair(tts, voices, plain):
    g = np.random.default_rng(5)
    durs = [1.3, 2.0, 0.9, 1.6]
    toks = [[int(t) for t in g.integers(1, 198, size=n)] for n in (7, 12, 5, 9)]
    rp = Repair(1, tau_token=plain["tau"], max_span=225, margin=0)
    kw = dict(token_lists=toks, durations=durs, seed=3, max_batch=3, repair=rp)
    out, pieces, mended = tts.synthesize_long(voices[1], return_pieces=True, return_repair=True, **kw)
    print(f"\n[long repair] kept {[int(m[0][0]) for m in mended]} (bad, free) {[m[1][0].tolist() for m in mended]}")
    assert len(pieces) == len(mended) == 4 and all(isinstance(q, Piece) for q in pieces)
    assert np.array_equal(tts.render_long(pieces, max_batch=3), out)               # the repaired latents, joined again: bit for bit
    assert np.array_equal(tts.synthesize_long(voices[1], **kw), out)                # asking for less changes nothing
    plain_out, plain_pieces = tts.synthesize_long(voices[1], return_pieces=True, **{k: v for k, v in kw.items() if k != "repair"})
    for q, q0, (kept, counts, before, after) in zip(pieces, plain_pieces, mended):
        assert kept.shape == (1,) and counts.shape == (1, 2) and 0 <= counts[0, 1] <= q.latents.shape[0]
        if not kept[0]:                                                             # a piece that was not replaced is the plain piece
            assert q.latents.tobytes() == q0.latents.tobytes() and before.tobytes() == after.tobytes()
        else:
            assert after[0] < before[0] and counts[0, 1] > 0 and q.latents.tobytes() != q0.latents.tobytes()
    # with takes in front, and the words on the repaired alignment
    out2, words, pieces2, taken, mended2 = tts.synthesize_long(voices[1], return_words=True, return_pieces=True, takes=2, return_takes=True,
                                                               return_repair=True, **kw)
    assert len(taken) == len(mended2) == 4 and np.array_equal(tts.render_long(pieces2, max_batch=3), out2)
    for i, (k, seed, tot, ft) in enumerate(taken):
        assert mended2[i][2].tobytes() == tot[k: k + 1].tobytes() and pieces2[i].seed == seed
