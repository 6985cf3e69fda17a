"""fp64 references, an error bound and edge-case inputs for the three softmax implementations (test infrastructure, not product
code): attention_img.hip (DMA + MFMA, the product's kernel), attention.hip (fp32 VALU) and align.hip's attn_text_mass (the tap).

* exact(...)            the fp64 restatement of dit.py:95-119 on raw projections (what tests/test_kernels_gpu.py calls _attn_ref);
                        also returns the logits and probabilities of every (b, h, n).
* as_computed(fmt, ..)  the same operation in fp64 ON THE OPERANDS AS THE KERNEL HOLDS THEM: every operand evaluated in fp64, cast
                        to fp32, rounded into the image format of common.hpp; the products the kernel forms (no lo x lo at the split
                        format); keys at the kernel's padded positions in 64-key chunks with the kernel's online softmax (P rounded
                        to the format relative to the RUNNING maximum, the row sum from the unrounded p).  fmt "fp32": no rounding
                        (the VALU kernel).  tap_as_computed: the tap's softmax on the same operands.
* bound(fmt, ref)       per-element bound on |kernel - as_computed|, from the reference's own quantities and the format units.
* mut_*                 eight wrong versions of as_computed (the slips the GPU tests are there to catch); tests/test_attn_ref_cpu.py
                        shows that each of them breaks the bound.
* build_case            seeded inputs of the case families A..E at the shapes of CASES.

Every constant below is a format unit or comes from the reasoning written next to it; none was read off a GPU run.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict

import torch

# ---- the bound's constants ---------------------------------------------------------------------------------------------------------
SAFETY = 4.0            # the ONE safety factor on the whole bound (first-order analysis, worst-case-to-typical slack)
U24 = 2.0 ** -24        # half an fp32 ulp, relative
UNIT = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8, "bf16x3": 2.0 ** -16, "fp32": 2.0 ** -24}   # rounding unit of P (and of the stored output)
F16_SUB = 2.0 ** -24    # smallest fp16 subnormal: absolute rounding unit of a probability below 2^-14
# logit error, in units of 2^-24 sum_d |q_d k_d|: the fp32 operand prep of q and k (rsq, two products, the rotation's fma, the
# scale: <= 4 roundings each = 8) + the fp32 accumulation of the products (dh <= 128 additions, each rounding <= 2^-24 of the
# partial sum; errors of mixed sign add like a random walk: sqrt(128) ~ 11.3 -> 12)
C_DOT = 20.0
# exp argument, in units of 2^-24 |s - m|: the subtraction (1), the product with log2(e) inside __expf (1), log2(e) itself (1)
C_EXP = 3.0
C_EXPULP = 2.0          # one exp evaluation: v_exp_f32 is ~1 ulp = 2 half-ulps (times the number of exps on a key's way: chunks + 1)
C_FLOOR = 8.0           # fp32 roundings behind the sum: 1 / l, two products, the sigmoid's rcp + exp (~4), the stored pair
# The kernel evaluates q^ and k^ in fp32 BEFORE it rounds them into the format (common.hpp QkPrep), as_computed in fp64.  The two
# values differ by the fp32 roundings of the preparation, in units of 2^-24 |x|: the sum of squares (pairwise, halved by the square
# root: 2), fmaf(ss, 1 / dh, eps) and the constant 1 / dh (halved: 1), v_rsq_f32 (1 ulp: 2), x rstd, x w (2), the rotation's fma and
# its inner product (2), the constant 1 / sqrt(dh) and the product with it (2) = 11 -> 12.  Where the fp64 value lies within that
# distance of a rounding tie of the format, the kernel may hold the NEIGHBOURING format value: a whole format ulp off, not 2^-24.
C_PREP = 12.0

KC, QT = 64, 32         # key chunk / query tile of attention_img_kernel
FMTS = ("fp32", "bf16x3", "f16", "bf16")


def pad8(n: int) -> int:
    return (n + 7) // 8 * 8


# ---- exact -------------------------------------------------------------------------------------------------------------------------
def _operands(qkvg, qw, kw, eps, rope, rot, H, dh, q_scale_pow=0):
    """fp64: q^ (head RMSNorm x w, RoPE, x dh^(-q_scale_pow/2)), k^, v as (B,H,N,dh); sigmoid(gate) as (B,N,D)"""
    B, N, _ = qkvg.shape
    D = H * dh
    x = qkvg.double()
    q, k, v, g = (x[..., i * D:(i + 1) * D].reshape(B, N, H, dh) for i in range(4))
    rms = lambda t, w: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    q, k = rms(q, qw), rms(k, kw)

    def rot_pairs(t):
        a = rope.double()[:N, :rot][None, :, None, 0::2]
        te, to = t[..., 0:rot:2], t[..., 1:rot:2]
        out = t.clone()
        out[..., 0:rot:2] = te * a.cos() - to * a.sin()
        out[..., 1:rot:2] = to * a.cos() + te * a.sin()
        return out
    q, k = rot_pairs(q).transpose(1, 2), rot_pairs(k).transpose(1, 2)
    if q_scale_pow:
        q = q * float(dh) ** (-0.5 * q_scale_pow)
    return q, k, v.transpose(1, 2), torch.sigmoid(g.reshape(B, N, D))


def exact(qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt):
    """torch restatement of dit.py:95-119 on raw projections (fp64) -> (out (B,N,D), logits (B,H,N,Ktot), probabilities)."""
    B, N, _ = qkvg.shape
    q, k, v, sg = _operands(qkvg, qw, kw, eps, rope, rot, H, dh)
    keys, vals, masks = [k], [v], [ms if ms is not None else torch.ones(B, N, dtype=torch.bool)]
    for kk, vv, mm in ((kr, vr, mr), (kt, vt, mt)):
        if kk is not None:
            keys.append(kk.double()); vals.append(vv.double())
            masks.append(mm if mm is not None else torch.ones(B, kk.shape[2], dtype=torch.bool))
    K, V, Mk = torch.cat(keys, 2), torch.cat(vals, 2), torch.cat(masks, 1)
    s = q @ K.transpose(-1, -2) / dh ** 0.5
    s = s.masked_fill(~Mk[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.nan_to_num(p, nan=0.0)
    o = (p @ V).transpose(1, 2).reshape(B, N, H * dh)
    return o * sg, s, p


# ---- the image formats of common.hpp -----------------------------------------------------------------------------------------------
def round_fmt(x: torch.Tensor, fmt: str):
    """fp64 value -> fp32 -> the format: (hi, lo) as fp64 (lo = 0 for the single formats).  f16: RNE, saturating at +-65504
    (cvt_pk_f16_sat); bf16: RNE; bf16x3: hi = bf16(x), lo = bf16(x - hi) (split1)."""
    x = x.float()
    if fmt == "fp32":
        return x.double(), torch.zeros_like(x, dtype=torch.float64)
    if fmt == "f16":
        return x.clamp(-65504.0, 65504.0).half().double(), torch.zeros_like(x, dtype=torch.float64)
    hi = x.bfloat16().float()
    if fmt == "bf16":
        return hi.double(), torch.zeros_like(x, dtype=torch.float64)
    assert fmt == "bf16x3", fmt
    lo = (x - hi).bfloat16().float()
    return hi.double(), lo.double()


def tie_slack(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """how far the held value of x moves when x moves by C_PREP 2^-24 |x| (the fp32 preparation error): 0 for nearly every element
    of a single format, one format ulp for an element next to a rounding tie; at the split format an ulp of lo (<= 2^-16 |x|)"""
    if fmt == "fp32":
        return torch.zeros_like(x)           # (no format rounding: the preparation error itself is in C_DOT)
    held = lambda t: sum(round_fmt(t, fmt))
    h0, w = held(x), C_PREP * U24
    return torch.maximum((held(x * (1 + w)) - h0).abs(), (held(x * (1 - w)) - h0).abs())


def _prod(ah, al, bh, bl):
    """a . b^T as the kernel forms it: hi hi + lo hi + hi lo, never lo lo"""
    bt = bh.transpose(-1, -2)
    return ah @ bt + al @ bt + ah @ bl.transpose(-1, -2)


def layout(fmt: str, N: int, R: int, P: int):
    """key positions as the kernel walks them: [0, Np) self | [Np, Np + Rp) reference | [Np + Rp, Kpos) text, then the rest of the
    last 64-key chunk.  The VALU kernel (fmt fp32) has no pad columns inside the range, only the tail of its last chunk."""
    pad = (lambda n: n) if fmt == "fp32" else pad8
    Np, Rp, Pp = pad(N), pad(R), pad(P)
    Kpos = Np + Rp + Pp
    nch = max(1, (Kpos + KC - 1) // KC)
    pos = torch.cat([torch.arange(N), Np + torch.arange(R), Np + Rp + torch.arange(P)])   # logical key -> position
    return SimpleNamespace(Np=Np, Rp=Rp, Pp=Pp, Kpos=Kpos, nch=nch, KP=nch * KC, pos=pos, N=N, R=R, P=P)


def pad_slots(L) -> Dict[str, int]:
    """the positions that hold no key: first pad column of each part, first position behind Kpos in the last chunk"""
    out = {}
    if L.Np > L.N: out["self"] = L.N
    if L.Rp > L.R: out["ref"] = L.Np + L.R
    if L.Pp > L.P: out["text"] = L.Np + L.Rp + L.P
    if L.KP > L.Kpos: out["tail"] = L.Kpos
    return out


def _staged(fmt, inp, q_scale_pow=1):
    """operands in the format at the kernel's key positions"""
    qkvg, qw, kw, eps, rope, rot, H, dh, kr, vr, kt, vt, ms, mr, mt = inp
    B, N, _ = qkvg.shape
    R = 0 if kr is None else kr.shape[2]
    P = 0 if kt is None else kt.shape[2]
    L = layout(fmt, N, R, P)
    q, k, v, sg = _operands(qkvg, qw, kw, eps, rope, rot, H, dh, q_scale_pow)
    ks, vs = [k], [v]
    masks = [ms if ms is not None else torch.ones(B, N, dtype=torch.bool)]
    for kk, vv, mm in ((kr, vr, mr), (kt, vt, mt)):
        if kk is not None:
            ks.append(kk.double()); vs.append(vv.double())     # cross keys arrive normalised and carry no RoPE; cross_pack rounds them
            masks.append(mm if mm is not None else torch.ones(B, kk.shape[2], dtype=torch.bool))
    qh, ql = round_fmt(q, fmt)
    kh_, kl_ = round_fmt(torch.cat(ks, 2), fmt)
    vh_, vl_ = round_fmt(torch.cat(vs, 2), fmt)
    gh, gl = round_fmt(sg, fmt)
    z = lambda: torch.zeros(B, H, L.KP, dh, dtype=torch.float64)
    kh, kl, vh, vl, dk = z(), z(), z(), z(), z()
    for dst, src in ((kh, kh_), (kl, kl_), (vh, vh_), (vl, vl_)):
        dst[:, :, L.pos] = src
    dk[:, :, L.pos[:N]] = tie_slack(k, fmt)                      # (cross keys arrive as numbers and are only rounded: no slack)
    valid = torch.zeros(B, L.KP, dtype=torch.bool)
    valid[:, L.pos] = torch.cat(masks, 1)
    return SimpleNamespace(L=L, B=B, N=N, H=H, dh=dh, qh=qh, ql=ql, kh=kh, kl=kl, vh=vh, vl=vl, gate=gh + gl, valid=valid,
                           masks=masks, dq=tie_slack(q, fmt), dk=dk)


def _f32(x):
    return x.float().double()


def _online(fmt, st, mut=None, arg=None, logits32=False):
    """attention_img_kernel::compute_chunk + finish in fp64 (every row at once).  `mut` selects one of the wrong versions."""
    L, B, H, N, dh = st.L, st.B, st.H, st.N, st.dh
    valid, vh, vl = st.valid.clone(), st.vh, st.vl
    if mut == "pad_valid":
        valid[:, arg] = True                                        # (K = V = 0 there: logit 0)
    elif mut == "mask_byte":
        b, pos = arg
        valid[b, pos] = True
    elif mut == "swap_masks":
        ms, mr, mt = st.masks                                       # (needs both cross parts)
        fit = lambda m, n: m[:, torch.arange(n) % m.shape[1]]       # byte j of the other part's mask, wrapped to this part's length
        valid = torch.zeros_like(valid)
        valid[:, L.pos] = torch.cat([ms, fit(mt, L.R), fit(mr, L.P)], 1)
    elif mut == "v_off_by_one":
        vh, vl = torch.roll(vh, -1, 2), torch.roll(vl, -1, 2)       # key j multiplies the V row of key j + 1
    s = _prod(st.qh, st.ql, st.kh, st.kl)
    if logits32:                                                    # (an fp32 accumulation, for the CPU stand-in of a correct kernel)
        s = _prod(st.qh.float(), st.ql.float(), st.kh.float(), st.kl.float()).double()
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    NEG = torch.full((B, H, N), float("-inf"), dtype=torch.float64)
    m_run = NEG.clone()
    if mut == "carried_max":                                        # reset() forgets m_run: query n starts from the final maximum of n - 32
        m_run[:, :, QT:] = s.max(-1).values[:, :, :-QT]
    l_run = torch.zeros(B, H, N, dtype=torch.float64)
    o = torch.zeros(B, H, N, dh, dtype=torch.float64)
    dead_lead = (~valid[:, :KC].any(1))[:, None, None].expand(B, H, N)
    for c in range(L.nch):
        sc = s[..., c * KC:(c + 1) * KC]
        m_new = torch.maximum(m_run, sc.max(-1).values)
        live = m_new != float("-inf")
        m_safe = torch.where(live, m_new, torch.zeros_like(m_new))
        alpha = torch.where(live & (m_run != float("-inf")), torch.exp(torch.where(m_run == float("-inf"), m_safe, m_run) - m_safe),
                            torch.where(live, torch.zeros_like(m_new), torch.ones_like(m_new)))
        p = torch.where(torch.isfinite(sc) & live[..., None], torch.exp(sc - m_safe[..., None]), torch.zeros_like(sc))
        if mut == "dead_chunk_nan":                                 # no `live` guard: exp(-inf - -inf)
            p = torch.where(live[..., None], p, torch.full_like(p, float("nan")))
        p = _f32(p)                                                 # (an fp32 exp: underflows below 2^-149)
        ph, pl = round_fmt(p, fmt)
        if mut == "no_rescale":
            alpha = torch.ones_like(alpha)
        l_run = l_run * alpha + p.sum(-1)
        vt_h, vt_l = vh[:, :, c * KC:(c + 1) * KC], vl[:, :, c * KC:(c + 1) * KC]
        o = o * alpha[..., None] + ph @ vt_h + ph @ vt_l + pl @ vt_h
        m_run = m_new
    inv = torch.where(l_run > 0, 1.0 / torch.where(l_run > 0, l_run, torch.ones_like(l_run)), torch.zeros_like(l_run))
    if mut == "dead_chunk_zero":                                    # a row whose first chunk is dead is taken for a dead row
        inv = torch.where(dead_lead, torch.zeros_like(inv), inv)
    out = (o * inv[..., None]).transpose(1, 2).reshape(B, N, H * dh) * st.gate
    return out, s, valid


def as_computed(fmt: str, *inp):
    """-> namespace: out (B,N,D) and everything bound() needs (logits s at the kernel's key positions, p, the operands as held)."""
    st = _staged(fmt, inp)
    out, s, valid = _online(fmt, st)
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    return SimpleNamespace(fmt=fmt, out=out, s=s, p=p, valid=valid, st=st)


def tap_as_computed(fmt: str, *inp):
    """attn_text_mass on the same operand images: logits from the whole held value (hi + lo) of q and k, an fp32 softmax, the mean
    over heads of the probabilities of the text keys; exactly 0 on frames that mask_self excludes.  -> namespace with mass (B,N,P)"""
    assert fmt != "fp32"
    return tap_of(fmt, _staged(fmt, inp))


def tap_of(fmt, st, logits32=False):
    L = st.L
    q, k = st.qh + st.ql, st.kh + st.kl
    s = (q.float() @ k.float().transpose(-1, -2)).double() if logits32 else q @ k.transpose(-1, -2)
    s = s.masked_fill(~st.valid[:, None, None, :], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    T0 = L.Np + L.Rp
    mass = p[..., T0:T0 + L.P].mean(1) * st.masks[0][:, :, None].double()
    return SimpleNamespace(fmt=fmt, mass=mass, s=s, p=p, valid=st.valid, st=st, q=q, k=k)


def stand_in(fmt: str, *inp):
    """What a CORRECT fp32 implementation may return (for the CPU file: the bounds must admit it).  q^, k^ and sigmoid(gate) are
    evaluated in fp32 (torch's own roundings, the approximate rsq / rcp / exp of the device stood in for by +-1 / +-2 ulp of seeded
    jitter) and THEN rounded to the format, so some operands land on the neighbouring format value, which as_computed does not
    model; fp32 logits.  Needs a rope table of zeros (every family has one).  -> namespace: out (B,N,D), mass (B,N,P) or None"""
    qkvg, qw, kw, eps, rope, rot, H, dh = inp[:8]
    assert not rope.any()
    B, N, D = qkvg.shape[0], qkvg.shape[1], H * dh
    gen = _gen(3)
    jit = lambda t, n: t * (1 + torch.randint(-n, n + 1, t.shape, generator=gen) * 2.0 ** -23)
    x = qkvg.float()
    q, k, _, g = (x[..., i * D:(i + 1) * D].reshape(B, N, H, dh) for i in range(4))
    prep = lambda t, w, sc: (((t * jit(torch.rsqrt((t * t).sum(-1, keepdim=True) * (1.0 / dh) + eps), 1)) * w) * sc).transpose(1, 2)
    st = _staged(fmt, inp)
    pos = st.L.pos[:N]
    st.qh, st.ql = round_fmt(prep(q, qw, 1.0 / dh ** 0.5).double(), fmt)
    st.kh[:, :, pos], st.kl[:, :, pos] = round_fmt(prep(k, kw, 1.0).double(), fmt)
    gh, gl = round_fmt(jit(1.0 / (1.0 + torch.exp(-g.reshape(B, N, D))), 2).double(), fmt)
    st.gate = gh + gl
    mass = tap_of(fmt, st, logits32=True).mass if st.L.P and fmt != "fp32" else None
    return SimpleNamespace(out=_online(fmt, st, logits32=True)[0], mass=mass)


# ---- the bound -----------------------------------------------------------------------------------------------------------------------
def _logit_slack(s, absqk, valid, nexp):
    """relative error of exp(s_j - m) as the kernel evaluates it, first order"""
    m = s.max(-1, keepdim=True).values
    gap = torch.where(valid[:, None, None, :] & torch.isfinite(m), m - s, torch.zeros_like(s))
    gap = torch.nan_to_num(gap, nan=0.0, posinf=0.0)
    return U24 * (C_DOT * absqk + C_EXP * gap + C_EXPULP * nexp)


def bound(fmt: str, ref) -> torch.Tensor:
    """|kernel - as_computed(fmt)| <= bound, per element (B,N,D):
         SAFETY * ( sigmoid(gate)_d * ( sum_j p_j eps_j |v_jd - o_d|  +  u_fmt sum_j p_j |v_jd|  [+ fp16: 2^-24 sum_j |v_jd| / l] )
                    + C_FLOOR 2^-24 max_j |v_j| )
       eps_j = 2^-24 (C_DOT sum_d |q_d k_jd| + C_EXP |s_j - m| + C_EXPULP (chunks + 1)); sums and the maximum over the live keys."""
    st, L = ref.st, ref.st.L
    B, H, N, dh = st.B, st.H, st.N, st.dh
    q, k, v = st.qh + st.ql, st.kh + st.kl, st.vh + st.vl
    eps = _logit_slack(ref.s, q.abs() @ k.abs().transpose(-1, -2), ref.valid, L.nch + 1)
    w = ref.p * eps                                                   # (B,H,N,KP); p = 0 on dead keys
    o = ref.p @ v
    first = torch.empty(B, H, N, dh, dtype=torch.float64)
    for b in range(B):                                                # (B,H,N,KP,dh) at once would be gigabytes at B = 33
        first[b] = (w[b][..., None] * (v[b][:, None] - o[b][:, :, None]).abs()).sum(2)
    vlive = v.abs() * ref.valid[:, None, :, None]
    tot = first + UNIT[fmt] * (ref.p @ v.abs())
    if fmt == "f16":
        lsum = torch.nan_to_num(torch.exp(ref.s - ref.s.max(-1, keepdim=True).values), nan=0.0).sum(-1).clamp_min(1.0)
        tot = tot + F16_SUB * vlive.sum(2)[:, :, None, :] / lsum[..., None]
    floor = C_FLOOR * U24 * vlive.amax((2, 3))                        # (B,H)
    to_bnd = lambda t: t.transpose(1, 2).reshape(B, N, H * dh)
    return SAFETY * (to_bnd(tot) * st.gate + to_bnd(floor[:, :, None, None].expand(B, H, N, dh)))


def tap_bound(ref, ties=True) -> torch.Tensor:
    """the same logit slack applied to p itself: |dp_j| <= p_j (eps_j + sum_k p_k eps_k), averaged over heads, plus fp32 ulps.
    The tap has no P rounding term that would cover an operand that the kernel holds one format ulp away from as_computed's (see
    C_PREP), so here eps_j also carries that: (sum_d (dq_d k_jd)^2 + (q_d dk_jd)^2)^(1/2) with dq, dk = tie_slack of q^, k^ (errors
    of mixed sign, added like the random walk of C_DOT; a single format has at most a few such elements in a row, and then this is
    their plain sum to within sqrt(2)).  0 on a row without an element next to a tie.  ties=False: without it (the CPU file shows
    that a correct fp32 implementation then leaves the bound)."""
    L, st = ref.st.L, ref.st
    eps = _logit_slack(ref.s, ref.q.abs() @ ref.k.abs().transpose(-1, -2), ref.valid, 2)
    if ties:
        eps = eps + (st.dq.square() @ ref.k.square().transpose(-1, -2) + ref.q.square() @ st.dk.square().transpose(-1, -2)).sqrt()
    dp = ref.p * (eps + (ref.p * eps).sum(-1, keepdim=True))
    T0 = L.Np + L.Rp
    return SAFETY * (dp[..., T0:T0 + L.P].mean(1) + C_FLOOR * U24) * ref.st.masks[0][:, :, None].double()


# ---- the eight slips: each returns what a kernel with that slip would compute ------------------------------------------------------
def mut_pad_valid(fmt, inp, slot="self"):
    """1. a pad position counted as a valid key with K = V = 0"""
    st = _staged(fmt, inp)
    return _online(fmt, st, "pad_valid", pad_slots(st.L)[slot])[0]


def mut_tap_pad_valid(fmt, inp, slot="self"):
    """1. for the tap: the mass with that pad position counted as a key"""
    st = _staged(fmt, inp)
    st.valid[:, pad_slots(st.L)[slot]] = True
    return tap_of(fmt, st).mass


def mut_mask_byte(fmt, inp, b=0, which=0):
    """2. one mask byte ignored: the `which`-th masked key of batch row b counts"""
    st = _staged(fmt, inp)
    real = torch.zeros(st.L.KP, dtype=torch.bool); real[st.L.pos] = True
    dead = torch.nonzero(real & ~st.valid[b]).flatten()
    return _online(fmt, st, "mask_byte", (b, int(dead[which])))[0]


def mut_swap_masks(fmt, inp):
    """3. the masks of the reference and the text keys swapped"""
    return _online(fmt, _staged(fmt, inp), "swap_masks")[0]


def mut_no_rescale(fmt, inp):
    """4. O and l not rescaled when the running maximum moves at a chunk boundary"""
    return _online(fmt, _staged(fmt, inp), "no_rescale")[0]


def mut_carried_max(fmt, inp):
    """5. the running maximum carried over from the previous 32-query tile"""
    return _online(fmt, _staged(fmt, inp), "carried_max")[0]


def mut_dead_chunk(fmt, inp, how="nan"):
    """6. a dead leading chunk leaves NaN (how = "nan") or output 0 (how = "zero") for the live keys behind it"""
    return _online(fmt, _staged(fmt, inp), "dead_chunk_" + how)[0]


def mut_v_off_by_one(fmt, inp):
    """7. every key's V row off by one key"""
    return _online(fmt, _staged(fmt, inp), "v_off_by_one")[0]


def mut_scale(fmt, inp, times=2):
    """8. 1 / sqrt(dh) applied twice (times = 2) or not at all (times = 0)"""
    return _online(fmt, _staged(fmt, inp, q_scale_pow=times))[0]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
# case -> (dh, rot, N, R, P, B, H): the smallest shapes at which each path of attention_img_kernel exists
CASES = {1: (64, 64, 64, 0, 0, 3, 2),        # DHP = 64, one full chunk, no cross part
         2: (120, 64, 61, 3, 5, 3, 2),       # Kpos 80: pad columns inside chunk 0, the cross part straddles the chunk boundary
         3: (120, 64, 65, 50, 57, 3, 2),     # Kpos 192, 3 chunks: resident (vm2) at f16 / bf16, streaming at bf16x3
         4: (128, 128, 100, 60, 81, 3, 2),   # Kpos 256, 4 full chunks: vm3, the LDS slot limit at f16
         5: (120, 64, 130, 70, 90, 3, 2),    # Kpos 304, 5 chunks: streaming everywhere, chunk_mask per chunk, 5 query tiles
         6: (120, 64, 40, 3, 5, 33, 8)}      # B H tiles = 528 > 2 x 256: a workgroup walks two query tiles against keys staged once
EPS = 1e-6


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit(t):
    return t / t.norm(dim=-1, keepdim=True)


def _near(d, cos, noise):
    """unit vector at cosine `cos` to the unit vector d, the rest along the part of `noise` orthogonal to d"""
    r = _unit(noise - (noise * d).sum(-1, keepdim=True) * d)
    return cos * d + math.sqrt(1.0 - cos * cos) * r


def _pack(qdir, kdir, vall, gate, g, dh, N, R, P, ms, mr, mt):
    """directions -> the hook's inputs.  Self rows are raw projections (sqrt(dh) x unit vector: RMS 1, so q^ = g u sqrt(dh) / sqrt(dh));
    cross keys arrive normalised: g sqrt(dh) x unit vector.  rope table of zeros, norm weights g x ones."""
    B, H = qdir.shape[:2]
    sq = math.sqrt(dh)
    rows = lambda t: t.transpose(1, 2).reshape(B, N, H * dh)
    qkvg = torch.cat([rows(qdir * sq), rows(kdir[:, :, :N] * sq), rows(vall[:, :, :N]), rows(gate)], -1).float().contiguous()
    w = torch.full((H, dh), float(g))
    kr = vr = kt = vt = None
    if R:
        kr, vr = (g * sq * kdir[:, :, N:N + R]).float().contiguous(), vall[:, :, N:N + R].float().contiguous()
    if P:
        kt, vt = (g * sq * kdir[:, :, N + R:]).float().contiguous(), vall[:, :, N + R:].float().contiguous()
    return (qkvg, w, w.clone(), EPS, None, None, H, dh, kr, vr, kt, vt, ms, mr if R else None, mt if P else None)


def build_case(family: str, case: int, seed: int = 0):
    """-> (inputs of the hooks in the order of exact(), info).  info.winner (B,H,N) = logical key index of the planted winner (or -1)."""
    dh, rot, N, R, P, B, H = CASES[case]
    B = {"B": 4, "C": 7}.get(family, B)     # B: three decoy parts + a dead row; C: five kill patterns + a dead row + a normal row
    Kt = N + R + P
    gen = _gen(1000 * case + 17 * seed + sum(map(ord, family)))
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    L = layout("f16", N, R, P)
    kpos = L.pos.tolist()
    rope = torch.zeros(N, rot)
    info = SimpleNamespace(family=family, case=case, winner=None, runner=None, g=3, L=L)
    ms, mr, mt = torch.ones(B, N, dtype=torch.bool), torch.ones(B, R, dtype=torch.bool), torch.ones(B, P, dtype=torch.bool)
    vall = (torch.rand(B, H, Kt, dh, generator=gen, dtype=torch.float64) * 8 - 4)
    gate = rn(B, H, N, dh)
    g = 3

    def all_masked(b):
        ms[b] = False; mr[b] = False; mt[b] = False

    if family in ("A0", "A1"):
        # one winner: query class c = n mod ncls points at the key at specials[c]; a runner-up 30 below in an earlier (A0) / later (A1) chunk
        sp = [i for i in (0, 63, 64, 127, N - 1) if i < N]
        if R: sp += [N, N + R - 1]
        if P: sp += [N + R, Kt - 1]
        sp = list(dict.fromkeys(sp))
        ncls = len(sp)
        d = _unit(rn(B, H, ncls, dh))
        kdir = _unit(rn(B, H, Kt, dh))
        kdir[:, :, sp] = d
        used = set(sp)
        cos_ru = 1.0 - 30.0 / (g * g * math.sqrt(dh))
        ru = [-1] * ncls
        for c, wi in enumerate(sp):
            cw = kpos[wi] // KC
            want = [cw - 1, cw + 1] if family == "A0" else [cw + 1, cw - 1]
            for cr in want:
                cand = [i for i in range(Kt) if kpos[i] // KC == cr and i not in used]
                if 0 <= cr < L.nch and cand:
                    i = cand[(7 * c + 3) % len(cand)]
                    used.add(i)
                    ru[c] = i
                    kdir[:, :, i] = _near(d[:, :, c], cos_ru, rn(B, H, dh))
                    break
        cls = torch.arange(N) % ncls
        qdir = d[:, :, cls]
        info.winner = torch.tensor(sp)[cls][None, None].expand(B, H, N).clone()
        info.runner = torch.tensor(ru)[cls][None, None].expand(B, H, N).clone()
        all_masked(B - 1)
        info.winner[B - 1] = -1
    elif family == "B":
        # masked decoy: the winner at cosine 0.8, a decoy at cosine 1.0 with V = 1e4 masked through mask_self / mask_ref / mask_text
        # (batch rows 0 / 1 / 2), two query classes per row; the last batch row has every key masked
        kdir = _unit(rn(B, H, Kt, dh))
        d = _unit(rn(B, H, 2, dh))
        plan = [((N, Kt - 1), (1, N - 2)),                                   # decoys among the self keys
                ((0, N - 1), (N, N + R - 1)),                                # ... the reference keys
                ((63 if N > 64 else N // 2, N + R - 1), (N + R, Kt - 1))]    # ... the text keys
        info.winner = torch.full((B, H, N), -1)
        cls = torch.arange(N) % 2
        for b, (wins, decoys) in enumerate(plan):
            for c in range(2):
                kdir[b, :, wins[c]] = _near(d[b, :, c], 0.8, rn(H, dh))
                kdir[b, :, decoys[c]] = d[b, :, c]
                vall[b, :, decoys[c]] = 1e4
                for m, lo_ in ((ms, 0), (mr, N), (mt, N + R)):
                    if lo_ <= decoys[c] < lo_ + m.shape[1]:
                        m[b, decoys[c] - lo_] = False
            info.winner[b] = torch.tensor(wins)[cls][None]
        qdir = d[:, :, cls]
        all_masked(B - 1)
    elif family in ("C", "D"):
        # every key near -u (a broad softmax far from logit 0).  D: every query near +u: all real logits <= -40, a pad position (logit 0)
        # would take the row.  C: queries of even 32-tiles near -u (logits ~ +70), of odd tiles near +u (~ -70), and masks that kill
        # whole chunks, one pattern per batch row.
        u = _unit(rn(B, H, 1, dh))
        kdir = _unit(-u + 0.6 * _unit(rn(B, H, Kt, dh)))
        if family == "D":
            qdir = _unit(u + 0.3 * _unit(rn(B, H, N, dh)))
            ms[1, N - 5:] = False
            if R: mr[1, 0] = False
            if P: mt[1, P // 2] = False
            all_masked(B - 1)
        else:
            sign = torch.where((torch.arange(N) // QT) % 2 == 0, -1.0, 1.0).double()[None, None, :, None]
            qdir = _unit(sign * u + 0.6 * _unit(rn(B, H, N, dh)))
            cat = torch.ones(B, Kt, dtype=torch.bool)
            kp = torch.tensor(kpos)
            cat[0, kp < 64] = False                                          # keys 0..63
            cat[1, kp < 128] = False                                         # keys 0..127
            cat[2, (kp >= 64) & (kp < 128)] = False                          # keys 64..127 only
            cat[3, :N + R] = False                                           # every self and reference key: only text is live
            cat[4, :Kt - 1] = False                                          # everything except the single key P - 1
            cat[5] = False                                                   # a dead row next to ...
            ms, mr, mt = cat[:, :N].clone(), cat[:, N:N + R].clone(), cat[:, N + R:].clone()   # ... row 6, a normal one
    elif family == "E":
        # moderate peaks: the Gaussian projections of the older tests with norm weights of 2 (logits within about +-16), all masks ragged
        g = 2
        gen = _gen(20 + case)
        rf = lambda *s: torch.randn(*s, generator=gen)
        D = H * dh
        qkvg = rf(B, N, 4 * D)
        w = torch.full((H, dh), 2.0)
        ms[0, N - N // 4:] = False
        if B > 2: ms[1, N - 3:] = False
        kr = vr = kt = vt = None
        if R:
            kr, vr = 2 * rf(B, H, R, dh), rf(B, H, R, dh)
            mr[0, R // 2:] = False; mr[1, 0] = False
        if P:
            kt, vt = 2 * rf(B, H, P, dh), rf(B, H, P, dh)
            mt[0, P // 3] = False; mt[1, P - 2:] = False
        all_masked(B - 1)
        info.g = 2
        return (qkvg, w, w.clone(), EPS, rope, rot, H, dh, kr, vr, kt, vt, ms, mr if R else None, mt if P else None), info
    else:
        raise ValueError(family)
    inp = list(_pack(qdir, kdir, vall, gate, g, dh, N, R, P, ms, mr, mt))
    inp[4], inp[5] = rope, rot
    return tuple(inp), info


# (family, case) pairs the GPU file runs: A..D where there is a cross part and more than one chunk (and dh 128), A0 also where a
# workgroup walks two tiles; E everywhere
GRID = [(f, c) for c in (2, 3, 4, 5) for f in ("A0", "A1", "B", "C", "D")] + [("A0", 6)] + [("E", c) for c in (1, 2, 3, 4, 5, 6)]
