"""CPU: tests/helpers/attn_ref.py is right and its bound discriminates.

The GPU file (tests/test_attention_edges_gpu.py) asserts |kernel - as_computed(fmt)| <= bound(fmt) per element.  Here, without a
device: exact() is the reference the older attention tests use; the format emulation rounds like common.hpp; the bound admits the
correct computation (as_computed("fp32") against exact); the case families have the properties they are named for; and each of
the eight slips breaks the bound on a named family, at every format — the proof that the GPU assertions can fail.  Every family at
its smallest shape (case 2; E also at case 1).  The tap's bound admits a correct fp32 tap only with its term for operands next to a
rounding tie, and a pad position counted as a key still breaks it."""
import functools

import pytest
import torch

from tests.helpers import attn_ref as R

SMALL = 2


@functools.lru_cache(maxsize=None)
def _case(family, case=SMALL):
    return R.build_case(family, case)


@functools.lru_cache(maxsize=None)
def _ref(family, fmt, case=SMALL):
    ref = R.as_computed(fmt, *_case(family, case)[0])
    return ref, R.bound(fmt, ref)


def _old_inputs(B, N, H, dh, rot, R_, P, seed=20):
    """the inputs of tests/test_kernels_gpu.py::test_attention"""
    rand = lambda *s, seed: torch.randn(*s, generator=torch.Generator().manual_seed(seed))
    D = H * dh
    qkvg = rand(B, N, 4 * D, seed=seed)
    qw, kw = 1 + 0.2 * rand(H, dh, seed=seed + 1), 1 + 0.2 * rand(H, dh, seed=seed + 2)
    inv = 1.0 / (1e4 ** (torch.arange(0, rot, 2).float() / rot))
    rope = (torch.arange(N).float()[:, None] * inv[None]).repeat_interleave(2, -1).contiguous()
    ms = torch.ones(B, N, dtype=torch.bool); ms[-1, N - N // 4:] = False
    kr, vr = rand(B, H, R_, dh, seed=seed + 3), rand(B, H, R_, dh, seed=seed + 4)
    mr = torch.ones(B, R_, dtype=torch.bool); mr[0, R_ // 2:] = False
    kt, vt = rand(B, H, P, dh, seed=seed + 5), rand(B, H, P, dh, seed=seed + 6)
    mt = torch.ones(B, P, dtype=torch.bool); mt[-1, :] = False
    return qkvg, qw, kw, 1e-6, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt


def test_exact_is_the_reference_of_the_older_tests_and_equals_an_independent_restatement():
    from tests import test_kernels_gpu as T
    inp = _old_inputs(2, 75, 8, 120, 64, 15, 30)
    out, s, p = R.exact(*inp)
    assert torch.equal(T._attn_ref(*inp), out), "test_kernels_gpu._attn_ref is not attn_ref.exact"
    # independent: complex-number rotation, torch's own scaled_dot_product_attention, in fp64
    qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt = inp
    B, N, D = qkvg.shape[0], qkvg.shape[1], H * dh
    x = qkvg.double().reshape(B, N, 4, H, dh)
    nrm = lambda t, w: t / (t.square().mean(-1, keepdim=True) + eps).sqrt() * w.double()

    def rotate(t):
        z = torch.view_as_complex(t[..., :rot].reshape(B, N, H, rot // 2, 2).contiguous())
        z = z * torch.polar(torch.ones(N, rot // 2, dtype=torch.float64), rope.double()[:, 0::2])[None, :, None]
        return torch.cat([torch.view_as_real(z).reshape(B, N, H, rot), t[..., rot:]], -1)
    q, k = rotate(nrm(x[:, :, 0], qw)).transpose(1, 2), rotate(nrm(x[:, :, 1], kw)).transpose(1, 2)
    K = torch.cat([k, kr.double(), kt.double()], 2)
    V = torch.cat([x[:, :, 2].transpose(1, 2), vr.double(), vt.double()], 2)
    M = torch.cat([ms, mr, mt], 1)[:, None, None, :].expand(B, H, N, -1)
    o = torch.nn.functional.scaled_dot_product_attention(q, K, V, attn_mask=M)
    want = torch.nan_to_num(o, nan=0.0).transpose(1, 2).reshape(B, N, D) * torch.sigmoid(x[:, :, 3].reshape(B, N, D))
    assert float((out - want).abs().max()) < 1e-12
    assert s.shape == p.shape == (B, H, N, 75 + 15 + 30) and float((p.sum(-1) - 1).abs().max()) < 1e-12


def test_format_emulation_rounds_like_common_hpp():
    x = torch.tensor([1e6, -7e4, 65504.0, 65519.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -26], dtype=torch.float64)
    hi, lo = R.round_fmt(x, "f16")
    assert hi.tolist() == [65504.0, -65504.0, 65504.0, 65504.0, 1.0, 1 + 2.0 ** -9, 0.0] and not lo.any()   # saturating, ties to even
    hi, lo = R.round_fmt(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3e38], dtype=torch.float64), "bf16")
    assert hi.tolist()[:2] == [1.0, 1 + 2.0 ** -6] and torch.isfinite(hi).all() and not lo.any()
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(100000, generator=g, dtype=torch.float64) * torch.exp(4 * torch.randn(100000, generator=g, dtype=torch.float64))).float().double()
    hi, lo = R.round_fmt(x, "bf16x3")
    assert torch.equal(hi, x.float().bfloat16().double()) and torch.equal(lo, (x - hi).float().bfloat16().double())
    assert bool(((hi + lo - x).abs() <= 2.0 ** -16 * x.abs()).all())
    hi, lo = R.round_fmt(x, "fp32")
    assert torch.equal(hi, x) and not lo.any()
    # the split product has no lo x lo term
    a, b = R.round_fmt(torch.tensor([[1 + 2.0 ** -9]], dtype=torch.float64), "bf16x3"), R.round_fmt(torch.tensor([[1 + 2.0 ** -9]], dtype=torch.float64), "bf16x3")
    assert float(R._prod(a[0], a[1], b[0], b[1])) == 1 + 2.0 ** -8


@pytest.mark.parametrize("family,case", [("A0", 2), ("A1", 2), ("B", 2), ("C", 2), ("D", 2), ("E", 2), ("E", 1)])
def test_fp32_as_computed_is_within_the_bound_of_exact(family, case):
    inp, _ = _case(family, case)
    ref, bd = _ref(family, "fp32", case)
    ex = R.exact(*inp)[0]
    ratio = ((ref.out - ex).abs() / bd.clamp_min(1e-300)).max()
    print(f"\n[attn ref] {family} case {case}: |as_computed(fp32) - exact| / bound = {float(ratio):.3g}")
    assert torch.isfinite(ref.out).all() and float(ratio) <= 1.0
    for fmt in ("bf16x3", "f16", "bf16"):   # the operand rounding the bound does NOT contain is visible at the format's unit, not beyond
        out = _ref(family, fmt, case)[0].out
        assert torch.isfinite(out).all() and float((out - ex).abs().max()) < 64 * R.UNIT[fmt] * max(1.0, float(ex.abs().max()))


@functools.lru_cache(maxsize=None)
def _stand_in(family, fmt, case=SMALL):
    return R.stand_in(fmt, *_case(family, case)[0])


@pytest.mark.parametrize("family,case", [("A0", 2), ("A1", 2), ("B", 2), ("C", 2), ("D", 2), ("E", 2), ("E", 1), ("C", 5), ("D", 5), ("E", 5)])
def test_a_correct_fp32_implementation_stays_within_the_bound_at_every_format(family, case):
    inp, _ = _case(family, case)
    for fmt in R.FMTS:
        ref, bd = _ref(family, fmt, case)
        err = (_stand_in(family, fmt, case).out - ref.out).abs()
        ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bd).max())
        print(f"\n[attn ref] {family} case {case}: fp32 stand-in at {fmt}: worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0, f"{family} case {case} {fmt}: {ratio:.3f}"


TAP_STAND_IN = [("A0", 2), ("B", 2), ("C", 2), ("D", 2), ("E", 2), ("D", 4), ("C", 5), ("E", 5)]


@pytest.mark.parametrize("family,case", TAP_STAND_IN)
def test_a_correct_fp32_tap_stays_within_the_tap_bound_at_every_format(family, case):
    """The tap has no P rounding term, so an operand that a correct fp32 preparation rounds to the neighbouring format value (its
    fp64 value lies next to a rounding tie) shows in full: without the tie term of tap_bound the stand-in leaves the bound (D case 4
    at bf16: 4.55 at (b, n, p) = (0, 99, 36); C case 5: 4.36 at bf16, 2.77 at f16), with it every ratio is below 0.25.  The term is 0
    on nearly every row at the single formats, so the bound there is the plain fp32 logit slack."""
    inp, _ = _case(family, case)
    worst_plain = 0.0
    for fmt in R.FMTS[1:]:
        ref = R.tap_as_computed(fmt, *inp)
        err = (_stand_in(family, fmt, case).mass - ref.mass).abs()
        ratio = lambda bd: float(torch.where(err == 0, torch.zeros_like(err), err / bd).max())
        bd, bd_plain = R.tap_bound(ref), R.tap_bound(ref, ties=False)
        with_ties, plain = ratio(bd), ratio(bd_plain)
        grow = (bd / bd_plain)[bd_plain > 0]
        print(f"\n[attn ref] {family} case {case}: tap bound with / without the tie term at {fmt}: max {float(grow.max()):.2f}, "
              f"mean {float(grow.mean()):.3f}, median {float(grow.median()):.3f}")
        if fmt == "bf16x3":     # lo has a tie within reach on about a third of the elements, each worth <= 2^-16 |x|: a random walk of
            # sqrt(2 dh / 3) ~ 9 such steps against the base slack's 20 x 2^-24 sum |q k|: the bound grows by about half, nowhere by 4
            assert float(grow.max()) <= 4.0 and float(grow.mean()) <= 1.5
        else:
            assert float(grow.median()) <= 1.5      # (D case 2 at f16: 1.34, elsewhere below 1.12)
        worst_plain = max(worst_plain, plain)
        print(f"\n[attn ref] {family} case {case}: fp32 tap stand-in at {fmt}: worst error / bound = {with_ties:.3f} (without the tie term {plain:.3f})")
        assert with_ties <= 1.0, f"{family} case {case} {fmt}: {with_ties:.3f}"
        if fmt != "bf16x3":     # a single format: an element next to a tie is rare (fp32 error / format ulp = C_PREP 2^-13 resp. 2^-16)
            st = ref.st
            rows = ((st.dq > 0).any(-1)[..., None] | (st.dk > 0).any(-1)[:, :, None, :]).double().mean()
            assert float((st.dq > 0).double().mean()) < 2 * R.C_PREP * R.U24 / R.UNIT[fmt] * 2 and float(rows) < 1.0
    if (family, case) in (("D", 4), ("C", 5)):
        assert worst_plain > 1.0, "the tie term is not what admits the correct tap here"


def test_a_pad_position_counted_as_a_key_breaks_the_tap_bound():
    inp, _ = _case("D")
    for fmt in R.FMTS[1:]:
        ref = R.tap_as_computed(fmt, *inp)
        bd = R.tap_bound(ref)
        for slot in R.pad_slots(ref.st.L):
            over = (R.mut_tap_pad_valid(fmt, inp, slot) - ref.mass).abs() > bd
            print(f"\n[attn ref] tap, pad position ({slot}) counted as a key at {fmt}: {int(over.any(-1).sum())} frames over the bound")
            assert int(over.any(-1).sum()) >= int(inp[12][:-1].sum()), (fmt, slot)      # every live frame of the live batch rows


# ---- the families have the properties they are named for ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["A0", "A1"])
def test_family_a_one_winner(family):
    inp, info = _case(family)
    out, s, p = R.exact(*inp)
    B, H, N = info.winner.shape
    live = info.winner >= 0
    w = info.winner.clamp_min(0)[..., None]
    sw = s.gather(3, w)[..., 0]
    rest = s.scatter(3, w, float("-inf"))
    ru = info.runner
    has = live & (ru >= 0)
    sr = s.gather(3, ru.clamp_min(0)[..., None])[..., 0]
    assert bool(has.any()) and float(((sw - sr)[has] - 30).abs().max()) < 0.5, "runner-up is not 30 below the winner"
    rest = rest.scatter(3, torch.where(has, ru, info.winner).clamp_min(0)[..., None], float("-inf"))
    margin = (sw - rest.max(-1).values)[live]
    print(f"\n[attn ref] {family}: winner logit {float(sw[live].min()):.1f}, margin over every other key >= {float(margin.min()):.1f}")
    assert float(margin.min()) >= 60.0 and float(sw[live].min()) > 9 * 120 ** 0.5 - 1
    # both orders exist: the runner-up's chunk is before (A0) / behind (A1) the winner's wherever such a chunk exists
    pos = info.L.pos
    cw, cr = pos[info.winner.clamp_min(0)] // R.KC, pos[ru.clamp_min(0)] // R.KC
    first = (cr < cw)[has] if family == "A0" else (cr > cw)[has]
    assert bool(first.any())
    # output = sigmoid(gate) v_winner, to the bound; the tap puts the whole text mass on a text winner
    qkvg, H_, dh = inp[0], inp[6], inp[7]
    D = H_ * dh
    Vall = torch.cat([qkvg.double()[..., 2 * D:3 * D].reshape(B, N, H_, dh).transpose(1, 2), inp[9].double(), inp[11].double()], 2)
    vw = Vall.gather(2, info.winner.clamp_min(0)[..., None].expand(B, H, N, dh))
    want = vw.transpose(1, 2).reshape(B, N, D) * torch.sigmoid(qkvg.double()[..., 3 * D:]) * live[:, 0, :, None]
    for fmt in R.FMTS:
        ref, bd = _ref(family, fmt)
        tol = bd + 4 * R.UNIT[fmt] * want.abs()      # (v and the gate as held differ from the raw ones by a rounding each)
        assert bool(((ref.out - want).abs() <= tol).all()), fmt
    tap = R.tap_as_computed("f16", *inp)
    T0 = info.L.N + info.L.R
    text_w = (info.winner >= T0).all(1) & live[:, 0]
    assert bool(text_w.any())
    mass = tap.mass
    assert float((mass.sum(-1)[text_w] - 1).abs().max()) < 1e-9
    idx = (info.winner[:, 0] - T0).clamp_min(0)
    assert float((mass.gather(2, idx[..., None])[..., 0][text_w] - 1).abs().max()) < 1e-9
    assert not mass[-1].any()


def test_family_b_the_masked_decoy_holds_the_largest_logit():
    inp, info = _case("B")
    qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt = inp
    B = qkvg.shape[0]
    assert B == 4 and not ms[0].all() and ms[1].all() and not mr[1].all() and not mt[2].all() and not (ms[3].any() or mr[3].any() or mt[3].any())
    _, s_un, _ = R.exact(qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, None, None, None)
    _, s, p = R.exact(*inp)
    dead = ~torch.cat([ms, mr, mt], 1)
    for b in range(3):
        top = s_un[b].argmax(-1)                              # (H, N): the decoy, a masked key with V = 1e4
        assert bool(dead[b][top].all())
        sw = s[b].gather(2, info.winner[b][..., None])[..., 0]
        margin = sw - s[b].scatter(2, info.winner[b][..., None], float("-inf")).max(-1).values
        assert float((s_un[b].max(-1).values - sw).min()) > 15 and float(margin.min()) >= 35.0
    assert float(torch.cat([vr, vt], 2).abs().max()) == 1e4 and float(qkvg.abs().max()) == 1e4
    assert float(R.as_computed("f16", *inp).out.abs().max()) <= 4.0 + 1e-6     # nothing of the decoy's 1e4 in the right answer


def test_family_c_dead_chunks():
    inp, info = _case("C", 5)      # (case 5 has keys 64..127 and 128.. in different parts)
    ms, mr, mt = inp[12:15]
    L = info.L
    valid = torch.zeros(ms.shape[0], L.KP, dtype=torch.bool)
    valid[:, L.pos] = torch.cat([ms, mr, mt], 1)
    real = torch.zeros(L.KP, dtype=torch.bool); real[L.pos] = True
    assert not valid[0, :64].any() and bool(valid[0, 64:][real[64:]].all())
    assert not valid[1, :128].any() and bool(valid[1, 128:][real[128:]].all())
    assert not valid[2, 64:128].any() and bool(valid[2, :64][real[:64]].all()) and bool(valid[2, 128:][real[128:]].all())
    assert not (ms[3].any() or mr[3].any()) and bool(mt[3].all())
    assert int(valid[4].sum()) == 1 and bool(mt[4, -1])
    assert not valid[5].any() and bool(valid[6][real].all())
    ref, _ = _ref("C", "f16", 5)
    assert not ref.out[5].any() and bool(ref.out[6].any()) and torch.isfinite(ref.out).all()
    # rows of neighbouring 32-query tiles sit ~140 logits apart: a running maximum that survives reset() underflows every exp
    m = ref.s[6].max(-1).values
    assert float((m[:, :32].min() - m[:, 32:64].max())) > 104


def test_family_d_every_real_logit_is_far_below_a_pad_positions_zero():
    inp, info = _case("D")
    _, s, p = R.exact(*inp)
    L = info.L
    assert float(s[torch.isfinite(s)].max()) <= -40.0
    assert L.Np != L.N and L.Rp != L.R and L.Pp != L.P and L.Kpos % R.KC != 0
    assert 0.0 < float(p[:2].max()) < 0.99        # a broad softmax, not one winner


def test_family_e_moderate_peaks():
    inp, info = _case("E", 5)
    _, s, p = R.exact(*inp)
    fin = s[torch.isfinite(s)]
    assert 12 < float(fin.max()) < 24 and -24 < float(fin.min()) < -12
    live = torch.isfinite(s).any(-1)
    rng = torch.where(torch.isfinite(s), s, torch.full_like(s, float("inf"))).min(-1).values
    assert float((s.max(-1).values - rng)[live].max()) > 20       # alpha reaches e^-20
    ms, mr, mt = inp[12:15]
    assert all(not m[0].all() and m[0].any() for m in (ms, mr, mt))


# ---- each slip breaks the bound ----------------------------------------------------------------------------------------------------
SLOTS = ("self", "ref", "text", "tail")
MUTATIONS = [
    # (name, the family it is shown on, function(fmt, inp), formats)
    *[(f"1 pad position ({s}) counted as a key", "D", (lambda s: lambda f, i: R.mut_pad_valid(f, i, s))(s),
       R.FMTS if s == "tail" else R.FMTS[1:]) for s in SLOTS],      # (the VALU kernel has no pad columns inside its key range)
    ("2 one mask byte ignored", "B", R.mut_mask_byte, R.FMTS),
    ("3 reference and text masks swapped", "B", R.mut_swap_masks, R.FMTS),
    ("4 no rescale when the running max moves", "A0", R.mut_no_rescale, R.FMTS),
    ("5 running max carried over from the previous query tile", "C", R.mut_carried_max, R.FMTS),
    ("6 dead leading chunk leaves NaN", "C", lambda f, i: R.mut_dead_chunk(f, i, "nan"), R.FMTS),
    ("6 dead leading chunk leaves output 0", "C", lambda f, i: R.mut_dead_chunk(f, i, "zero"), R.FMTS),
    ("7 V row off by one key", "A0", R.mut_v_off_by_one, R.FMTS),
    ("8 1/sqrt(dh) applied twice", "E", lambda f, i: R.mut_scale(f, i, 2), R.FMTS),
    ("8 1/sqrt(dh) not applied", "E", lambda f, i: R.mut_scale(f, i, 0), R.FMTS),
]


@pytest.mark.parametrize("name,family,fn,fmts", MUTATIONS, ids=[m[0].replace(" ", "_") for m in MUTATIONS])
def test_each_slip_breaks_the_bound(name, family, fn, fmts):
    inp, info = _case(family)
    for fmt in fmts:
        ref, bd = _ref(family, fmt)
        out = fn(fmt, inp)
        over = ~((out - ref.out).abs() <= bd)                      # (NaN counts as over)
        if family == "C":
            over[5] = False                                        # the dead row does not count: the slip must hurt live keys
        rows = torch.nonzero(over.any(-1))
        ratio = torch.nan_to_num((out - ref.out).abs() / bd.clamp_min(1e-300), nan=float("inf"))[over]
        first = tuple(rows[0].tolist()) if len(rows) else None
        print(f"\n[attn ref] slip {name!r} on family {family} at {fmt}: {len(rows)} rows over the bound, first (b, n) = {first}, "
              f"worst error / bound = {float(ratio.max()) if len(rows) else 0.0:.3g}")
        assert len(rows) > 0, f"{name}: family {family} at {fmt} stays inside the bound"
        # ... where a correct fp32 implementation of the same family at the same format is inside
        assert bool(((_stand_in(family, fmt).out - ref.out).abs() <= bd).all()), f"{name}: the stand-in leaves the bound on {family} at {fmt}"
