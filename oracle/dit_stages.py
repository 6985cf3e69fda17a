"""ORACLE (test infrastructure, NOT product code).

The DiT and the two condition encoders stated stage by stage in plain fp64, as the product's stage functions cut them
(smtts_test_dit_stage, include/smalltts_hip.h): the modulation table, the input embedding, one block at a time, the final
AdaLN and the velocity head; per encoder the input, one block at a time, the final norm, the output projection and the
cross K / V of the 12 DiT blocks.  Every operation is spelled out (the grouped conv as frame shifts, the softmax over
self + ref + text keys with its mask) rather than called from torch.nn.functional, so that the GPU tests compare each
kernel with arithmetic that shares none of its structure.  tests/test_dit_stages_oracle.py pins the composition of these
stages to oracle/dit_oracle.py (itself pinned to the reference's modules by the golden fixtures).

The angle tables (time sinusoid, RoPE) are formed in fp32 as the reference's modules form them; their sin / cos and
everything after runs in fp64.  Weights: a {name: tensor} dict in the reference's state_dict names, any float dtype.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

HIDDEN, HEADS, DH, NBLK, ROPE_DIM, FF = 960, 8, 120, 12, 64, 2400
MOD_PER_BLOCK = 6 * HIDDEN
MOD_LD = NBLK * MOD_PER_BLOCK + 2 * HIDDEN       # one modulation row: 12 x [sh_a sc_a tanh(g_a) sh_m sc_m tanh(g_m)] | final [scale shift]
CONV_K, CONV_G, CONV_PAD = 31, 16, 15
ENC = {"style": dict(prefix="style_encoder.blocks", layers=12, heads=8, dim=512, eps=1e-5, norm="style_encoder.norm.weight"),
       "text": dict(prefix="phoneme_embedding.blocks", layers=8, heads=4, dim=512, eps=1e-6, norm="phoneme_embedding.norm.weight")}


def _d(w, name):
    return w[name].to(torch.float64)


# ---- the rounding stand-in (default off) ----------------------------------------------------------------------------------------
# Engine::Site (engine.hpp) by weight name; presets as Engine::set_precision assigns them (SITE_COND stays split-bf16 under f16)
SITE_FMT = {"bf16x3": dict(dit_block="bf16x3", encoder="bf16x3", cross_kv="bf16x3", cond="bf16x3"),
            "f16": dict(dit_block="f16", encoder="f16", cross_kv="f16", cond="bf16x3"),
            "bf16": dict(dit_block="bf16", encoder="bf16", cross_kv="bf16", cond="bf16")}
_ROUND = None   # the active Rounding, or None: _lin is the plain fp64 product


def site_of(name: str) -> str:
    """the Engine::Site whose GEMM reads the linear `name` (no trailing .weight)"""
    if name.startswith("dit.transformer_blocks."):
        leaf = name.split(".", 3)[3]
        if leaf == "attn_norm.linear":
            return "cond"
        if leaf.startswith(("attn.to_k_ref", "attn.to_v_ref", "attn.to_k_text", "attn.to_v_text")):
            return "cross_kv"
        return "dit_block"
    if ".blocks." in name or name in ("style_encoder.out_proj", "dit.phoneme_proj"):
        return "encoder"
    return "cond"   # time MLP, emb_proj, norm_out, the latent in-projection, the velocity head, the style in-projection


class Rounding:
    """While active (`with Rounding(preset):`) _lin rounds BOTH operands of every product to the format the preset assigns to the
    site of that weight name (f16: RNE saturating at +-65504; bf16; split hi + lo without the lo x lo product), through round_fmt of
    tests/helpers/attn_ref.py, and forms the product in fp64.  One instance serves one weight dict (the rounded weights are kept by
    name); amax[site] is the largest |operand| a site has seen.

    This is a CONDITIONING PROXY built from the reference alone: it says how much harder a weight family or an input makes the
    same stage for operands of that width, relative to another family.  It is no model of the kernels: it rounds neither the
    attention images (q, k, V^T, the gate, P) nor the conv pos-embed, knows nothing of fp32 accumulation order or of the fp32
    residual stream, and does not form the LN-fold's (x - c)(1 + scale) image."""

    def __init__(self, preset: str):
        self.fmt = SITE_FMT[preset]
        self.wcache: Dict[str, tuple] = {}
        self.amax: Dict[str, float] = {}

    def __enter__(self):
        global _ROUND
        self.prev, _ROUND = _ROUND, self
        return self

    def __exit__(self, *exc):
        global _ROUND
        _ROUND = self.prev

    @staticmethod
    def off():
        """`with Rounding.off():` the plain fp64 product inside an active Rounding"""
        return _Off()

    def product(self, w, name, x):
        from tests.helpers.attn_ref import round_fmt
        site = site_of(name)
        fmt = self.fmt[site]
        if name not in self.wcache:
            self.wcache[name] = round_fmt(_d(w, name + ".weight"), fmt)
        wh, wl = self.wcache[name]
        xh, xl = round_fmt(x, fmt)
        self.amax[site] = max(self.amax.get(site, 0.0), float(x.abs().max()) if x.numel() else 0.0, float(wh.abs().max()))
        y = xh @ wh.t()
        return y + xl @ wh.t() + xh @ wl.t() if fmt == "bf16x3" else y


class _Off:
    def __enter__(self):
        global _ROUND
        self.prev, _ROUND = _ROUND, None

    def __exit__(self, *exc):
        global _ROUND
        _ROUND = self.prev


def _lin(w, name, x, bias=True, col_shift=0):
    """col_shift != 0 (near miss): the weight image moved by that many input columns"""
    if col_shift:
        y = x @ _d(w, name + ".weight").roll(col_shift, 1).t()
    else:
        y = x @ _d(w, name + ".weight").t() if _ROUND is None else _ROUND.product(w, name, x)
    return y + _d(w, name + ".bias") if bias else y


def silu(x):
    return x / (1 + torch.exp(-x))


def mish(x):
    return x * torch.tanh(torch.log1p(torch.exp(-x.abs())) + x.clamp_min(0))   # x tanh(softplus x), softplus without overflow


def layer_norm(x, eps=1e-6):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps)


def rms_norm(x, wgt, eps):
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * wgt


def rotate_pairs(x, ang):
    """(x[2i], x[2i+1]) rotated by ang[..., i]: the RoPE of dit.py:152-173 and style.py:21-25 / phonemes.py:79-83 alike."""
    c, s = torch.cos(ang), torch.sin(ang)
    xe, xo = x[..., 0::2], x[..., 1::2]
    out = torch.empty_like(x)
    out[..., 0::2] = xe * c - xo * s
    out[..., 1::2] = xo * c + xe * s
    return out


def rope_half_angles(n: int, dim: int) -> torch.Tensor:
    """(n, dim / 2) angles pos * 10000^(-2i / dim), formed in fp32 as the reference forms them"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
    return (torch.arange(n, dtype=torch.float32)[:, None] * inv[None, :]).to(torch.float64)


def attention(q, k, v, key_mask, scale):
    """q (B, H, Nq, d), k / v (B, H, Nk, d), key_mask (B, Nk) bool: masked softmax written out.  A row with no key gives 0."""
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    s = torch.where(key_mask[:, None, None, :], s, torch.full_like(s, -math.inf))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    p = torch.exp(s - m)
    den = p.sum(-1, keepdim=True)
    p = torch.where(den > 0, p / den.clamp_min(1e-300), torch.zeros_like(p))
    return torch.einsum("bhqk,bhkd->bhqd", p, v)


# ---- DiT `mod`: time sinusoid -> MLP -> emb_proj -> modulation table (model.py:16-30, dit.py:19-39) ---------------------------
def sinusoid(t, half_den: Optional[int] = None):
    half = 128
    den = half - 1 if half_den is None else half_den
    f = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(1e4) / den))
    e = (1e3 * t.to(torch.float32)[:, None] * f[None, :]).to(torch.float64)
    return torch.cat([torch.sin(e), torch.cos(e)], -1)


def mod_table(w, t, tanh_gates=True, half_den: Optional[int] = None):
    """-> (rows, MOD_LD) in the product's layout; the gates carry their tanh (dit.py:198, 201)"""
    temb = _lin(w, "time_embedding.mlp.2", silu(_lin(w, "time_embedding.mlp.0", sinusoid(t, half_den))))
    semb = silu(_lin(w, "dit.emb_proj.2", silu(_lin(w, "dit.emb_proj.0", temb))))
    parts = []
    for i in range(NBLK):
        m = _lin(w, f"dit.transformer_blocks.{i}.attn_norm.linear", semb)
        if tanh_gates:
            m = m.clone()
            m[:, 2 * HIDDEN:3 * HIDDEN] = torch.tanh(m[:, 2 * HIDDEN:3 * HIDDEN])
            m[:, 5 * HIDDEN:6 * HIDDEN] = torch.tanh(m[:, 5 * HIDDEN:6 * HIDDEN])
        parts.append(m)
    parts.append(_lin(w, "dit.norm_out.linear", semb))   # [scale | shift] (dit.py:37)
    return torch.cat(parts, -1)


def mod_rows(table, B, row0=0, rstride=0):
    """the modulation row of each utterance: row0 + b rstride"""
    return table.to(torch.float64)[torch.tensor([row0 + b * rstride for b in range(B)])]


# ---- DiT `embed`: latent in-projection + the grouped conv pos-embed (dit.py:215-253) ------------------------------------------
def grouped_conv(w, name, x, shift=0):
    """conv1d(groups 16, k 31, padding 15) over frames as explicit shifts: x (B, N, 960).  shift != 0 moves every tap (near miss)"""
    B, N, C = x.shape
    cpg = C // CONV_G
    wt = _d(w, name + ".weight").reshape(CONV_G, cpg, cpg, CONV_K)      # [g][out][in][tap]
    xp = torch.zeros(B, N + 2 * CONV_PAD + 2, CONV_G, cpg, dtype=torch.float64)
    xp[:, CONV_PAD + 1:CONV_PAD + 1 + N] = x.reshape(B, N, CONV_G, cpg)
    out = torch.zeros(B, N, CONV_G, cpg, dtype=torch.float64)
    for k in range(CONV_K):
        s = k + 1 + shift
        out += torch.einsum("bngi,goi->bngo", xp[:, s:s + N], wt[..., k])
    return out.reshape(B, N, C) + _d(w, name + ".bias")


def embed(w, x_t, mask, tap_shift=0, remask=True):
    m = mask.to(torch.float64)[..., None]
    h = _lin(w, "dit.input_embed.proj", x_t.to(torch.float64))
    p = "dit.input_embed.conv_pos_embed"
    c = mish(grouped_conv(w, p + ".conv1", h * m, tap_shift))
    if remask:
        c = c * m
    c = mish(grouped_conv(w, p + ".conv2", c, tap_shift))
    return c * m + h


# ---- DiT `blocks`: one block at a time (dit.py:95-135, 189-212) ---------------------------------------------------------------
def adaln(x, shift, scale):
    return layer_norm(x) * (1 + scale[:, None]) + shift[:, None]


def adaln_unshifted_f16(x, shift, scale):
    """near miss of the LN-fold before its row shift: the operand image x (1 + scale) rounded to fp16 around 0 instead of around the
    row mean, the mean / rstd correction applied after the product (gemm.hpp LnFoldIn)"""
    mu = x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
    img = (x * (1 + scale[:, None])).to(torch.float16).to(torch.float64)
    return (img - mu * (1 + scale[:, None])) * rstd + shift[:, None]


def adaln_fold_term_dropped(x, shift, scale):
    """near miss of the LN-fold epilogue rstd (acc - (mu - c) tab1) + tab0 + b without its (mu - c) tab1 term, c the previous row's
    mean (row 0: its own): every product W y of the image gains rstd (mu - c) W (1 + scale), stated here on y itself"""
    mu = x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-6)
    c = torch.cat([mu[:, :1], mu[:, :-1]], 1)
    return adaln(x, shift, scale) + rstd * (mu - c) * (1 + scale[:, None])


def adaln_scale_only(x, shift, scale):
    """near miss: scale in place of 1 + scale"""
    return layer_norm(x) * scale[:, None] + shift[:, None]


SLIP_NORMS = {"fold_term_dropped": adaln_fold_term_dropped, "scale_only": adaln_scale_only}


def block_mod(rows, l):
    """(sh_a, sc_a, tanh g_a, sh_m, sc_m, tanh g_m) of block l, each (B, 960), from the per-utterance modulation rows"""
    m = rows[:, l * MOD_PER_BLOCK:(l + 1) * MOD_PER_BLOCK]
    return [m[:, i * HIDDEN:(i + 1) * HIDDEN] for i in range(6)]


def final_mod(rows, swap=False):
    """(shift, scale) of the final AdaLN: the table holds [scale | shift] (dit.py:37)"""
    sc, sh = rows[:, NBLK * MOD_PER_BLOCK:NBLK * MOD_PER_BLOCK + HIDDEN], rows[:, NBLK * MOD_PER_BLOCK + HIDDEN:]
    return (sc, sh) if swap else (sh, sc)


def dit_block(w, l, x, mask, rows, cache, ang=None, q_scale=None, rope_layout="pairs", unshifted_f16=False, slip=None):
    """x (B, N, 960) -> x after block l.  cache: k_ref / v_ref (L, B, H, R, 120), ref_mask (B, R), k_text / v_text, ph_mask.
    q_scale, rope_layout, unshifted_f16: near misses; slip: one more, by name (a key of SLIP_NORMS: that AdaLN; "swap_qk_norm": the
    two head-norm weights exchanged; "abs_head_norm": |w| for w in both; "w2_col_shift": ff.w2 moved by one input column)"""
    B, N, _ = x.shape
    p = f"dit.transformer_blocks.{l}"
    sh_a, sc_a, g_a, sh_m, sc_m, g_m = block_mod(rows, l)
    norm = adaln_unshifted_f16 if unshifted_f16 else SLIP_NORMS.get(slip, adaln)
    y = norm(x, sh_a, sc_a)
    q = _lin(w, f"{p}.attn.to_q", y).reshape(B, N, HEADS, DH)
    k = _lin(w, f"{p}.attn.to_k_self", y).reshape(B, N, HEADS, DH)
    v = _lin(w, f"{p}.attn.to_v_self", y).reshape(B, N, HEADS, DH)
    qn, kn = _d(w, f"{p}.attn.q_norm.weight"), _d(w, f"{p}.attn.k_norm.weight")
    if slip == "swap_qk_norm":
        qn, kn = kn, qn
    if slip == "abs_head_norm":
        qn, kn = qn.abs(), kn.abs()
    q = rms_norm(q, qn, 1e-6)
    k = rms_norm(k, kn, 1e-6)
    a = rope_half_angles(N, ROPE_DIM) if ang is None else ang
    if rope_layout == "pairs":
        rot = lambda z: torch.cat([rotate_pairs(z[..., :ROPE_DIM], a[None, :, None, :]), z[..., ROPE_DIM:]], -1)
    else:   # near miss: rotate (i, i + 32) instead of (2i, 2i + 1)
        def rot(z):
            h = ROPE_DIM // 2
            c, s = torch.cos(a)[None, :, None, :], torch.sin(a)[None, :, None, :]
            z1, z2 = z[..., :h], z[..., h:ROPE_DIM]
            return torch.cat([z1 * c - z2 * s, z2 * c + z1 * s, z[..., ROPE_DIM:]], -1)
    q, k = rot(q), rot(k)
    kk = [k.transpose(1, 2)]
    vv = [v.transpose(1, 2)]
    km = [mask]
    for tag, mk in (("ref", "ref_mask"), ("text", "ph_mask")):
        if cache.get("k_" + tag) is not None and cache["k_" + tag].shape[3] > 0:
            kk.append(cache["k_" + tag][l].to(torch.float64))
            vv.append(cache["v_" + tag][l].to(torch.float64))
            km.append(cache[mk])
    o = attention(q.transpose(1, 2), torch.cat(kk, 2), torch.cat(vv, 2), torch.cat(km, 1),
                  1.0 / math.sqrt(DH) if q_scale is None else q_scale)
    o = o.transpose(1, 2).reshape(B, N, HIDDEN) * torch.sigmoid(_lin(w, f"{p}.attn.gate", y, False))
    o = _lin(w, f"{p}.attn.to_out.0", o, False) * mask.to(torch.float64)[..., None]
    x = x + g_a[:, None] * o
    h = norm(x, sh_m, sc_m)
    ff = _lin(w, f"{p}.ff.w2", silu(_lin(w, f"{p}.ff.w1", h)) * _lin(w, f"{p}.ff.w3", h), col_shift=int(slip == "w2_col_shift"))
    return x + g_m[:, None] * ff


def next_image(x, rows, l1, swap=False):
    """the AdaLN image the blocks [.., l1) leave for the next GEMM: block l1's attention AdaLN, or the final one"""
    if l1 < NBLK:
        sh, sc = block_mod(rows, l1)[:2]
    else:
        sh, sc = final_mod(rows, swap)
    return adaln(x, sh, sc)


def head(w, img, bias=True, col_shift=0):
    return _lin(w, "velocity", img, bias, col_shift)


# ---- encoders ---------------------------------------------------------------------------------------------------------------
def style_in(w, ref, with_scale=True):
    x = _lin(w, "style_encoder.in_proj", ref.to(torch.float64))
    return x * torch.exp(_d(w, "style_encoder.log_scale")) if with_scale else x


def text_in(w, ids):
    return _d(w, "phoneme_embedding.text_embedding.weight")[ids]


def enc_block(w, net, l, x, key_mask, rope_dims=None):
    """rope_dims: rotate only the first rope_dims of each head (near miss; the encoders rotate the whole head)"""
    c = ENC[net]
    p, H, eps = f"{c['prefix']}.{l}", c["heads"], c["eps"]
    B, S, D = x.shape
    dh = D // H
    h = rms_norm(x, _d(w, f"{p}.attention_norm.weight"), eps)
    q = _lin(w, f"{p}.attention.wq", h, False).reshape(B, S, H, dh)
    k = _lin(w, f"{p}.attention.wk", h, False).reshape(B, S, H, dh)
    v = _lin(w, f"{p}.attention.wv", h, False).reshape(B, S, H, dh)
    g = _lin(w, f"{p}.attention.gate", h, False)
    q = rms_norm(q, _d(w, f"{p}.attention.q_norm.weight"), eps)
    k = rms_norm(k, _d(w, f"{p}.attention.k_norm.weight"), eps)
    rd = dh if rope_dims is None else rope_dims
    a = rope_half_angles(S, rd)[None, :, None, :]
    q = torch.cat([rotate_pairs(q[..., :rd], a), q[..., rd:]], -1)
    k = torch.cat([rotate_pairs(k[..., :rd], a), k[..., rd:]], -1)
    o = attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), key_mask, 1.0 / math.sqrt(dh))
    x = x + _lin(w, f"{p}.attention.wo", o.transpose(1, 2).reshape(B, S, D) * torch.sigmoid(g), False)
    h = rms_norm(x, _d(w, f"{p}.mlp_norm.weight"), eps)
    return x + _lin(w, f"{p}.mlp.w2", silu(_lin(w, f"{p}.mlp.w1", h, False)) * _lin(w, f"{p}.mlp.w3", h, False), False)


def enc_image(w, net, x, l1):
    """the RMSNorm image the blocks [.., l1) leave: block l1's attention norm, or the final norm"""
    c = ENC[net]
    name = f"{c['prefix']}.{l1}.attention_norm.weight" if l1 < c["layers"] else c["norm"]
    return rms_norm(x, _d(w, name), c["eps"])


def enc_out(w, net, img, key_mask):
    y = _lin(w, "style_encoder.out_proj" if net == "style" else "dit.phoneme_proj", img)
    return y * key_mask.to(torch.float64)[..., None]


def cross_kv(w, net, seq, knorm=True, knorm_name="k_norm_cross"):
    """-> K, V (12, B, 8, S, 120): to_k / to_v of every DiT block, K through k_norm_cross (dit.py:80-93; knorm=False and
    knorm_name="k_norm", the self keys' weight: near misses)"""
    tag = "ref" if net == "style" else "text"
    B, S, _ = seq.shape
    ks, vs = [], []
    for i in range(NBLK):
        p = f"dit.transformer_blocks.{i}.attn"
        k = _lin(w, f"{p}.to_k_{tag}", seq).reshape(B, S, HEADS, DH)
        ks.append((rms_norm(k, _d(w, f"{p}.{knorm_name}.weight"), 1e-6) if knorm else k).transpose(1, 2))
        vs.append(_lin(w, f"{p}.to_v_{tag}", seq).reshape(B, S, HEADS, DH).transpose(1, 2))
    return torch.stack(ks), torch.stack(vs)


# ---- compositions (tests/test_dit_stages_oracle.py pins these to dit_oracle) -------------------------------------------------
def denoise_step(w, x_t, mask, t, cache, ph_mask) -> torch.Tensor:
    rows = mod_table(w, t)
    c = dict(cache, ph_mask=ph_mask)
    x = embed(w, x_t, mask)
    for l in range(NBLK):
        x = dit_block(w, l, x, mask, rows, c)
    return head(w, next_image(x, rows, NBLK))


def encode_conditions(w, ref, ref_len, ids, ph_mask) -> Dict[str, torch.Tensor]:
    R = ref.shape[1]
    ref_mask = torch.arange(R)[None, :] < ref_len.clamp(max=R)[:, None]
    out = {"ref_mask": ref_mask}
    for net, x, km in (("style", style_in(w, ref), ref_mask), ("text", text_in(w, ids), ph_mask)):
        for l in range(ENC[net]["layers"]):
            x = enc_block(w, net, l, x, km)
        seq = enc_out(w, net, enc_image(w, net, x, ENC[net]["layers"]), km)
        k, v = cross_kv(w, net, seq)
        tag = "ref" if net == "style" else "text"
        out["k_" + tag], out["v_" + tag] = k, v
        out["ref_seq" if net == "style" else "phoneme_mem"] = seq
    return out
