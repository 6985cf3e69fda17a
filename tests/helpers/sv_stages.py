"""The speaker verifier one launch at a time (tests/test_scorer_stages_gpu.py, tests/test_scorer_stages_cpu.py).

stages(model, taps, x, n, row) gives, for every launch of smtts_sv_embed (the slot names of engine_hooks.SCORER_TAPS["sv"]), the fp64
result of that launch alone and its rounding bound (tests/helpers/stage_bounds.py), computed by the parameters of the restatement's own
sub-modules (tests/helpers/sv_ref.py) from `taps`: the buffers the launches before it left.  With the device's taps that is teacher
forcing: a stage's reference starts from what the device itself fed that stage, so its error is the stage's own, whatever happened in
front.  With ref_taps (the same functions composed in order, nothing from a device) the last slot is the restatement's embedding.

A stage is what one launch computes.  sv_res2net is the whole 11-band chain in one launch; its tap holds every band's output, so band i is
held from the device's own band i - 1 (u_i = x_i + y_{i - 1}, one fp32 addition, repeated here exactly): eleven local bounds, no
bound grown through the chain.  The attention's TDNN takes the row constant from its tap and includes the tanh; the pooling includes
the asp_bn affine.  Everything is one row alone at its own length n >= 6, frames (n, C); what lies at and behind n is not looked at.

mut names a broken copy of one stage (the sharpness tests): "bf16" (both operands of the stage's product; "bf16:1" / "bf16:2" where
it has two), "edge" (edge repeat instead of reflect), "no_crow" (the row constant omitted), "uniform_std" (the uniform instead of the
weighted standard deviation).  Of a broken copy only the value means anything: its bound is taken from the unbroken call."""
import torch

from smalltts_amd.engine_hooks import SCORER_TAPS
from tests.helpers.stage_bounds import F, TINY, U, ULP, bf16, dot, f64, relu, sigmoid_lip
from tests.helpers.sv_ref import ASP_EPS

NAMES = SCORER_TAPS["sv"]
BN_EPS = 1e-5


def _fold(norm):
    """BatchNorm (eval) as scale, shift: what finalize folds in double and rounds once each"""
    bn = norm.norm
    sc = bn.weight / torch.sqrt(bn.running_var + BN_EPS)
    return sc, bn.bias - bn.running_mean * sc


def _affine(r, er, sc, sh):
    """fmaf(r, fl(sc), fl(sh)): the rounding of either folded constant, one of the result"""
    y = r * sc + sh
    return y, sc.abs() * er + U * ((r * sc).abs() + sh.abs() + y.abs())


def _gather(x, k, d, edge):
    """frames (n, C) -> (n, k C): tap j of frame t is frame t + (j - (k - 1) / 2) d, reflected about the row's own ends"""
    if k == 1:
        return x
    n = x.shape[0]
    cols = []
    for j in range(k):
        t = torch.arange(n) + (j - (k - 1) // 2) * d
        t = t.clamp(0, n - 1) if edge else torch.where(t < 0, -t, torch.where(t >= n, 2 * (n - 1) - t, t))
        cols.append(x[t])
    return torch.cat(cols, dim=1)


def tdnn(mod, x, mut=None, crow=None, tanh=False, cin=None):
    """conv (reflect), ReLU, BatchNorm [, + row constant in front of the ReLU, tanh behind] of frames x (n, C) -> (value, bound)"""
    W = mod.conv.conv.weight                       # (O, I, k)
    O, I, k = W.shape
    if cin is not None:                            # the attention's TDNN: its first cin input channels; the rest is the row constant
        W, I = W[:, :cin], cin
    d = mod.conv.conv.dilation[0]
    a = _gather(x, k, d, mut == "edge")
    w = W.permute(0, 2, 1).reshape(O, k * I)       # k index = tap * I + channel
    b = mod.conv.conv.bias
    if crow is not None:                           # bias + c is one addition of the kernel's, then one with the product
        v, e = dot(a, w, None, mut=mut)
        c = torch.zeros_like(crow) if mut == "no_crow" else crow
        A = a.abs() @ w.abs().T
        v = v + (b + c)
        e = e + U * (b + crow).abs() + U * (A + (b + crow).abs())
    else:
        v, e = dot(a, w, b, mut=mut)
    sc, sh = _fold(mod.norm)
    y, e = _affine(*relu(v, e), sc, sh)
    if tanh:
        y = torch.tanh(y)
        e = e + F["tanhf"] * ULP * y.abs()
    return y, e


def res2net(blk, x, y_dev, mut=None, exact=False):
    """The band chain: x (n, 768) the block's tdnn1, y_dev (n, 768) the launch's own tap, from which band i takes band i - 1.  exact:
    u_i = x_i + y_{i - 1} in double (the composition test); else as the kernel adds it, in fp32."""
    outs, errs = [x[:, :64]], [torch.zeros_like(x[:, :64])]       # band 0 passes through: a copy
    for j in range(1, 12):
        xj = x[:, 64 * j:64 * j + 64]
        if j == 1:
            u = xj
        elif exact:
            u = xj + y_dev[:, 64 * (j - 1):64 * j]
        else:
            u = (xj.float() + y_dev[:, 64 * (j - 1):64 * j].float()).double()
        y, e = tdnn(blk.res2net_block.blocks[j - 1], u, mut=mut)
        outs.append(y)
        errs.append(e)
    return torch.cat(outs, 1), torch.cat(errs, 1)


def se_gate(se, x, mut=None):
    """time mean, 768 -> 192, ReLU, 192 -> 768, sigmoid -> (value, bound), (768)"""
    n = x.shape[0]
    s = x.mean(0)
    es = n * U * x.abs().mean(0) + U * s.abs()
    h, eh = dot(s[None], se.conv1.conv.weight[:, :, 0], se.conv1.conv.bias, ea=es[None], mut="bf16" if mut == "bf16:1" else None)
    h, eh = relu(h, eh)
    g, eg = dot(h, se.conv2.conv.weight[:, :, 0], se.conv2.conv.bias, ea=eh, mut="bf16" if mut == "bf16:2" else None)
    y = torch.sigmoid(g)[0]
    return y, (sigmoid_lip(g, eg) * eg)[0] + F["sigmoid"] * ULP * y + TINY


def se_apply(x, gate, res, mut=None):
    gx = bf16(gate)[None] * bf16(x) if mut == "bf16" else gate[None] * x
    y = gx + res
    return y, U * ((gate[None] * x).abs() + (gate[None] * x + res).abs())


def _sqrt_eps(v, ev):
    """sqrt(max(v, eps)) and its bound for an error ev of v: sqrt a - sqrt b = (a - b) / (sqrt a + sqrt b), the smaller root taken at
    its least (not first order: a channel that is constant over time has v = 0 in the reference and a rounding's square on the device)"""
    s = torch.sqrt(v.clamp(min=ASP_EPS))
    lo = torch.sqrt((v - ev).clamp(min=ASP_EPS))
    return s, ev / (s + lo) + F["sqrtf"] * ULP * s


def _wstats(x, w, ew, n):
    """weighted mean and two-pass std over frames: x, w, ew (n, C); the weights sum to 1 -> (m, em, s, es)"""
    m = (w * x).sum(0)
    em = (ew * x.abs()).sum(0) + n * U * (w * x).abs().sum(0)
    dv = x - m
    edv = em + U * dv.abs()
    sq = dv * dv
    esq = 2 * dv.abs() * edv + edv * edv + U * (dv.abs() + edv) ** 2
    v = (w * sq).sum(0)
    ev = (ew * sq).sum(0) + (w * esq).sum(0) + n * U * v
    s, es = _sqrt_eps(v, ev)
    return m, em, s, es


def asp_stats(x):
    """uniform [mean ; std] over the row's frames -> (value, bound), (4608)"""
    n = x.shape[0]
    w = torch.full_like(x, 1.0 / n)
    m, em, s, es = _wstats(x, w, U * w, n)       # 1.0f / n: one rounding
    return torch.cat([m, s]), torch.cat([em, es])


def asp_pool(asp_bn, lg, x, mut=None):
    """softmax over the row's frames per channel, weighted mean and std, asp_bn -> (value, bound), (4608)"""
    n = x.shape[0]
    z = lg - lg.max(0).values
    p = torch.exp(z)
    rp = U * z.abs() + F["expf"] * ULP                     # relative, of one expf(lg - mx)
    l = p.sum(0)
    rl = (p * rp).sum(0) / l + n * U                       # of the sum, then of 1.0f / l and of the product with it
    w = p / l
    ew = w * (rp + rl + 2 * U) + TINY / l
    xv = bf16(x) if mut == "bf16" else x
    wv = bf16(w) if mut == "bf16" else w
    m, em, s, es = _wstats(x, w, ew, n)
    if mut == "bf16":
        m = (wv * xv).sum(0)
        s = torch.sqrt((wv * (xv - m) ** 2).sum(0).clamp(min=ASP_EPS))
    if mut == "uniform_std":
        s = torch.sqrt(((x - m) ** 2).mean(0).clamp(min=ASP_EPS))
    sc, sh = _fold(asp_bn)
    y, e = _affine(torch.cat([m, s]), torch.cat([em, es]), sc, sh)
    return y, e


def stages(model, taps, x, n, row=0, only=None, mut=None, exact=False):
    """{slot name: (fp64 value, bound)} of row `row` (n >= 6 frames) for the slots in `only` (default: all).  taps: {slot name: tensor
    (B, ...)}; x (B, N, 64) the call's latents.  mut: the broken copy, of the slots in `only`."""
    ec = model.ecapa
    t = lambda name: f64(taps[name][row, :n]) if taps[name].dim() == 3 else f64(taps[name][row])
    out = {}
    want = NAMES if only is None else only
    for name in want:
        if name == "blocks.0":
            out[name] = tdnn(ec.blocks[0], f64(x[row, :n]), mut=mut)
        elif name.startswith("blocks."):
            i, part = int(name.split(".")[1]), name.split(".")[2]
            blk = ec.blocks[i]
            prev = "blocks.0" if i == 1 else f"blocks.{i - 1}.out"
            if part == "tdnn1":
                out[name] = tdnn(blk.tdnn1, t(prev), mut=mut)
            elif part == "res2net":
                out[name] = res2net(blk, t(f"blocks.{i}.tdnn1"), t(name), mut=mut, exact=exact)
            elif part == "tdnn2":
                out[name] = tdnn(blk.tdnn2, t(f"blocks.{i}.res2net"), mut=mut)
            elif part == "gate":
                out[name] = se_gate(blk.se_block, t(f"blocks.{i}.tdnn2"), mut=mut)
            else:
                out[name] = se_apply(t(f"blocks.{i}.tdnn2"), t(f"blocks.{i}.gate"), t(prev), mut=mut)
        elif name == "mfa":
            out[name] = tdnn(ec.mfa, torch.cat([t(f"blocks.{i}.out") for i in (1, 2, 3)], 1), mut=mut)
        elif name == "stats":
            v, e = asp_stats(t("mfa"))
            out[name] = (asp_stats(bf16(t("mfa")))[0], e) if mut == "bf16" else (v, e)
        elif name == "crow":
            W = ec.asp.tdnn.conv.conv.weight[:, :, 0]
            out[name] = tuple(v[0] for v in dot(t("stats")[None], W[:, W.shape[1] // 3:], None, mut=mut))
        elif name == "att":
            out[name] = tdnn(ec.asp.tdnn, t("mfa"), mut=mut, crow=t("crow"), tanh=True, cin=t("mfa").shape[1])
        elif name == "logit":
            out[name] = dot(t("att"), ec.asp.conv.conv.weight[:, :, 0], ec.asp.conv.conv.bias, mut=mut)
        elif name == "pooled":
            out[name] = asp_pool(ec.asp_bn, t("logit"), t("mfa"), mut=mut)
        elif name == "emb":
            out[name] = tuple(v[0] for v in dot(t("pooled")[None], ec.fc.conv.weight[:, :, 0], ec.fc.conv.bias, mut=mut))
        else:
            raise KeyError(name)
    return out


@torch.no_grad()
def ref_taps(model, x, lengths, dtype=torch.float64):
    """The stage functions composed in order, every row alone: {slot name: (B, ...)} in the layout of the device's taps, NaN where the
    device writes nothing (at and behind a row's length; every slot but emb of a row under 6 frames), emb of such a row 0.0."""
    from smalltts_amd.engine_hooks import scorer_tap_shapes
    B, N = x.shape[:2]
    taps = {k: torch.full(sh, float("nan"), dtype=torch.float64) for k, sh in scorer_tap_shapes("sv", B, N).items()}
    for b, n in enumerate(int(v) for v in lengths):
        if n < 6:
            taps["emb"][b] = 0.0
            continue
        for name in NAMES:
            if name.endswith(".res2net"):          # band by band: band i reads band i - 1 of the slot being filled
                i = int(name.split(".")[1])
                xin = taps[f"blocks.{i}.tdnn1"][b, :n]
                y = torch.zeros(n, 768, dtype=torch.float64)
                for _ in range(11):
                    y = res2net(model.ecapa.blocks[i], xin, y, exact=True)[0]
                v = y
            else:
                v = stages(model, taps, x, n, b, only=[name], exact=True)[name][0]
            if taps[name].dim() == 3:
                taps[name][b, :n] = v
            else:
                taps[name][b] = v
    return {k: v.to(dtype) for k, v in taps.items()}
