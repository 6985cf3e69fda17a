"""The recogniser one launch at a time (tests/test_scorer_stages_gpu.py, tests/test_scorer_stages_cpu.py).

stages(model, taps, x, n, row) gives, for every launch of smtts_asr_logprobs (the slot names of engine_hooks.SCORER_TAPS["asr"]), the
fp64 result of that launch alone and its rounding bound (tests/helpers/stage_bounds.py), computed by the parameters of the
restatement's own sub-modules (tests/helpers/asr_ref.py) from `taps`, the buffers the launches before it left: teacher forcing with the
device's taps, the restatement itself with ref_taps (see tests/helpers/sv_stages.py).

A stage is what one launch computes: ffn1 is LayerNorm, 64 -> 1024, SiLU, 1024 -> 64 and the half-step residual; ffn2 the same and the
layer's final LayerNorm; qkv the attention's LayerNorm and in-projection (q times 1 / sqrt(4)); attn the 16 heads' softmax (a shift of
the scores by the device's own maximum cancels in the quotient: it is no error); proj the out-projection and the residual (which it
reads from the slot of ffn1: the launch updates that buffer in place); conv the whole conv module and its residual; logp the projection
to 198 classes and the log-softmax.  One row alone at its own length, T = 4 n frames (T, 64).

mut names a broken copy of one stage: "bf16" (both operands of its product; "bf16:1" ... where it has several, in order), "drop_key"
(the row's last key missing from the attention), "tap9" (the ninth conv tap missing at frames t = 55 mod 56), "full_step" (the
half-step 0.5 replaced by 1)."""
import torch

from smalltts_amd.engine_hooks import SCORER_TAPS
from tests.helpers.stage_bounds import F, SILU_LIP, TINY, U, ULP, bf16, dot, f64, sigmoid_lip

NAMES = SCORER_TAPS["asr"]
LN_EPS, BN_EPS = 1e-5, 1e-5
HEADS, DH = 16, 4


def layer_norm(ln, v, ev=None):
    """LayerNorm over 64 channels of frames v (T, 64) with error bound ev -> (value, bound)"""
    g, be = ln.weight, ln.bias
    C = v.shape[1]
    ev = torch.zeros_like(v) if ev is None else ev
    mu = v.mean(1, keepdim=True)
    emu = ev.mean(1, keepdim=True) + C * U * v.abs().mean(1, keepdim=True)
    d = v - mu
    ed = ev + emu + U * d.abs()
    var = (d * d).mean(1, keepdim=True)
    evar = (2 * d.abs() * ed + U * d * d).mean(1, keepdim=True) + C * U * var + U * (var + LN_EPS)
    r = 1.0 / torch.sqrt(var + LN_EPS)
    rel_r = evar / (2 * (var + LN_EPS)) + F["rsqrt"] * ULP
    t = d * r * g
    y = t + be
    e = (g * r).abs() * ed + t.abs() * rel_r + 2 * U * t.abs() + U * y.abs()
    return y, e


def silu(v, ev):
    y = v * torch.sigmoid(v)
    return y, SILU_LIP * ev + F["silu"] * ULP * y.abs()


def ffn(seq, xin, mut=None, final_ln=None):
    ln, l1, l2 = seq[0], seq[1], seq[4]
    a, ea = layer_norm(ln, xin)
    h, eh = dot(a, l1.weight, l1.bias, ea=ea, mut="bf16" if mut == "bf16:1" else None)
    h, eh = silu(h, eh)
    o, eo = dot(h, l2.weight, l2.bias, ea=eh, mut="bf16" if mut == "bf16:2" else None)
    step = 1.0 if mut == "full_step" else 0.5
    y = step * o + xin
    e = 0.5 * eo + U * (0.5 * o + xin).abs()
    if final_ln is not None:
        y, e = layer_norm(final_ln, y, e)
    return y, e


def qkv(layer, xin, mut=None):
    a, ea = layer_norm(layer.self_attn_layer_norm, xin)
    v, e = dot(a, layer.self_attn.in_proj_weight, layer.self_attn.in_proj_bias, ea=ea, mut=mut)
    sc = torch.ones(v.shape[1], dtype=v.dtype)
    sc[:64] = 0.5                                   # q / sqrt(head dim): exact
    return v * sc, e * sc


def attention_weights(qkv_t):
    """(16 heads, T queries, T keys) softmax of the tapped q (already scaled), k"""
    T = qkv_t.shape[0]
    q, k = (qkv_t[:, i * 64:(i + 1) * 64].reshape(T, HEADS, DH).permute(1, 0, 2) for i in (0, 1))
    return torch.softmax(q @ k.transpose(1, 2), dim=-1)


def attn(qkv_t, mut=None):
    T = qkv_t.shape[0]
    q, k, v = (qkv_t[:, i * 64:(i + 1) * 64].reshape(T, HEADS, DH).permute(1, 0, 2) for i in (0, 1, 2))   # (16, T, 4)
    qm, km = (bf16(q), bf16(k)) if mut == "bf16:1" else (q, k)
    s = qm @ km.transpose(1, 2)                                           # (16, Tq, Tk)
    es = DH * U * (q.abs() @ k.abs().transpose(1, 2))
    if mut == "drop_key":
        s = s[:, :, :-1]
    z = s - s.max(-1, keepdim=True).values
    p = torch.exp(z)
    w = p / p.sum(-1, keepdim=True)
    vv = v[:, :-1] if mut == "drop_key" else v
    o = (bf16(w) @ bf16(vv)) if mut == "bf16:2" else w @ vv
    # the bound, from the unbroken quantities
    s0 = q @ k.transpose(1, 2)
    z0 = s0 - s0.max(-1, keepdim=True).values
    p0 = torch.exp(z0)
    l0 = p0.sum(-1, keepdim=True)
    w0 = p0 / l0
    rp = es + U * z0.abs() + F["expf"] * ULP                              # relative, of one p
    rl = (w0 * rp).sum(-1, keepdim=True) + T * U                          # of the denominator
    o0 = w0 @ v
    rl = rl + T * TINY / l0                                               # (a p under the normal range)
    e = (w0 * rp + TINY / l0) @ v.abs() + T * U * (w0 @ v.abs()) + o0.abs() * (rl + 2 * U)
    return o.permute(1, 0, 2).reshape(T, 64), e.permute(1, 0, 2).reshape(T, 64)


def proj(layer, o, res, mut=None):
    v, e = dot(o, layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias, mut=mut)
    y = v + res
    return y, e + U * y.abs()


def conv(cm, xin, mut=None):
    seq = cm.sequential
    T = xin.shape[0]
    a, ea = layer_norm(cm.layer_norm, xin)
    pw, epw = dot(a, seq[0].weight[:, :, 0], seq[0].bias, ea=ea, mut="bf16" if mut == "bf16:1" else None)
    va, g = pw[:, :64], pw[:, 64:]
    sg = torch.sigmoid(g)
    glu = va * sg
    eglu = sg * epw[:, :64] + va.abs() * (sigmoid_lip(g, epw[:, 64:]) * epw[:, 64:] + F["sigmoid"] * ULP * sg + TINY) + U * glu.abs()
    dw, db = seq[2].weight[:, 0, :], seq[2].bias                          # (64, 9)
    K = dw.shape[1]
    pad = (K - 1) // 2
    z = torch.zeros(pad, 64, dtype=glu.dtype)
    gp, egp = torch.cat([z, glu, z]), torch.cat([z, eglu, z])
    d = db.expand(T, 64).clone()
    A = db.abs().expand(T, 64).clone()
    ed = torch.zeros_like(d)
    gm, dwm = (bf16(gp), bf16(dw)) if mut == "bf16:2" else (gp, dw)
    for j in range(K):
        term = gm[j:j + T] * dwm[:, j]
        if mut == "tap9" and j == K - 1:
            term = torch.where((torch.arange(T) % 56 == 55)[:, None], torch.zeros_like(term), term)
        d = d + term
        A = A + (gp[j:j + T] * dw[:, j]).abs()
        ed = ed + egp[j:j + T] * dw[:, j].abs()
    ed = ed + (K + 1) * U * A
    bn = seq[3]
    sc = bn.weight / torch.sqrt(bn.running_var + BN_EPS)
    sh = bn.bias - bn.running_mean * sc
    y = d * sc + sh
    ey = sc.abs() * ed + U * ((d * sc).abs() + sh.abs() + y.abs())
    s, es = silu(y, ey)
    o, eo = dot(s, seq[5].weight[:, :, 0], seq[5].bias, ea=es, mut="bf16" if mut == "bf16:3" else None)
    out = o + xin
    return out, eo + U * out.abs()


def head(lin, xin, mut=None):
    z, ez = dot(xin, lin.weight, lin.bias, mut=mut)
    z0 = dot(xin, lin.weight, lin.bias)[0]
    out = torch.log_softmax(z, dim=-1)
    zs = z0 - z0.max(-1, keepdim=True).values
    p = torch.exp(zs)
    s = p.sum(-1, keepdim=True)
    sm = p / s
    C = z0.shape[1]
    rs = (sm * (U * zs.abs() + F["expf"] * ULP)).sum(-1, keepdim=True) + C * U + C * TINY / s
    ls = torch.log(s)
    ref = torch.log_softmax(z0, dim=-1)
    e = ez + (sm * ez).sum(-1, keepdim=True) + U * zs.abs() + rs + F["logf"] * ULP * ls.abs() + U * ref.abs()
    return out, e


def upsample(dc, x, mut=None):
    w, b = dc.weight[:, 0, :], dc.bias                                    # (64, 4)
    n = x.shape[0]
    xr = x[:, None, :].expand(n, 4, 64)
    prod = (bf16(xr) * bf16(w.T)[None]) if mut == "bf16" else xr * w.T[None]
    y = (prod + b).reshape(4 * n, 64)
    t = (xr * w.T[None]).reshape(4 * n, 64)
    return y, U * (t.abs() + (t + b).abs())


def stages(model, taps, x, n, row=0, only=None, mut=None):
    """{slot name: (fp64 value, bound)} of row `row` (n >= 1 latent frames) for the slots in `only` (default: all)"""
    T = 4 * n
    t = lambda name: f64(taps[name][row, :T])
    out = {}
    for name in (NAMES if only is None else only):
        if name == "upsample":
            out[name] = upsample(model.upsample.deconv, f64(x[row, :n]), mut=mut)
        elif name == "logp":
            out[name] = head(model.proj, t(f"layers.{len(model.encoder.conformer_layers) - 1}.ffn2"), mut=mut)
        else:
            _, l, part = name.split(".")
            l = int(l)
            L = model.encoder.conformer_layers[l]
            prev = "upsample" if l == 0 else f"layers.{l - 1}.ffn2"
            if part == "ffn1":
                out[name] = ffn(L.ffn1.sequential, t(prev), mut=mut)
            elif part == "qkv":
                out[name] = qkv(L, t(f"layers.{l}.ffn1"), mut=mut)
            elif part == "attn":
                out[name] = attn(t(f"layers.{l}.qkv"), mut=mut)
            elif part == "proj":
                out[name] = proj(L, t(f"layers.{l}.attn"), t(f"layers.{l}.ffn1"), mut=mut)
            elif part == "conv":
                out[name] = conv(L.conv_module, t(f"layers.{l}.proj"), mut=mut)
            else:
                out[name] = ffn(L.ffn2.sequential, t(f"layers.{l}.conv"), mut=mut, final_ln=L.final_layer_norm)
    return out


@torch.no_grad()
def ref_taps(model, x, lengths, dtype=torch.float64):
    """The stage functions composed in order, every row alone, in the layout of the device's taps: NaN at and behind frame 4 n_b,
    logp 0.0 there."""
    from smalltts_amd.engine_hooks import scorer_tap_shapes
    B, N = x.shape[:2]
    taps = {k: torch.full(sh, float("nan"), dtype=torch.float64) for k, sh in scorer_tap_shapes("asr", B, N).items()}
    taps["logp"].zero_()
    for b, n in enumerate(int(v) for v in lengths):
        if n < 1:
            continue
        for name in NAMES:
            taps[name][b, :4 * n] = stages(model, taps, x, n, b, only=[name])[name][0]
    return {k: v.to(dtype) for k, v in taps.items()}
