"""Structured weight families, the inputs and cases of the weight-family tests, and the allowance factor A (test infrastructure,
not product code; numpy / torch only, no GPU).

Every engine of the suite is filled by weights.init_rule: zero-mean uniform matrices, norm weights 1 +- 0.2, small modulation
rows.  A trained checkpoint is not at hand, so these families put the STRUCTURE of one onto the synthetic state dict: a
common mode per matrix row, input columns of unequal scale, heavy tails, head-norm weights of both signs over two decades,
modulation parts that differ by orders of magnitude, and AdaLN-Zero.  They are synthetic structured weights, not a trained model.

family(sd, name, seed) is a lazy view of sd: a tensor is formed when it is read, from a generator keyed by (tensor name, family,
seed) alone, so a test that loads only stage_names() pays for those only.

Cases: one Case states a stage of tests/test_weight_families_gpu.py on seeded inputs: outputs(w) is its plain fp64 reference
(oracle/dit_stages.py), errors(got, ref) the per-row / per-utterance figures the GPU test bounds.  A (amplification) compares the
rounding stand-in of dit_stages (Rounding) under a family with the same stand-in under the shipped synthetic weights and the
plain inputs: A(row) = max(1, e_model(row) / e0), e0 the largest e_model of that case.  It is computed from the reference alone.
"""
from __future__ import annotations

import math
import re
from typing import Dict

import numpy as np
import torch

from oracle import dit_stages as DS
from smalltts_amd.weights import dit_param_specs, fnv1a64, synth_state_dict
from tests.test_dit_kernels_gpu import BOUND, _floor, _inputs, _lengths, _mask, _rel_rows, _rel_utt

SEED = 13
FAMILIES = ("zero", "common", "colscale", "heavy", "norms", "mod")
A_CAP = 8.0
# the families' constants
K = dict(common=0.1, colbase=8.0, normbase=4.0, neg=0.3, scale=(-0.99, 4.0), scale_pow=16, shift=3.0, gate=5.0)
F16_HEADROOM = 65504.0 / 4

_MOD_LIN = re.compile(r"(dit\.transformer_blocks\.\d+\.attn_norm\.linear|dit\.norm_out\.linear)\.(weight|bias)$")


def _is_norm(name):
    return name.endswith("norm.weight") or name.endswith("norm_cross.weight")


def _is_matrix(name, arr):
    return arr.ndim == 2 and name.endswith(".weight") and not _is_norm(name)


def changes(fam: str, name: str, arr) -> bool:
    """does family `fam` change the tensor `name`?"""
    if fam == "synth":
        return False
    if fam == "zero":
        return bool(_MOD_LIN.match(name))
    if fam in ("common", "colscale", "heavy"):
        return _is_matrix(name, arr)
    if fam == "norms":
        return _is_norm(name) or name == "style_encoder.log_scale"
    if fam == "mod":
        return bool(_MOD_LIN.match(name)) and name.endswith(".bias")
    raise KeyError(fam)


def _gen(name, fam, seed):
    return torch.Generator().manual_seed((fnv1a64(f"{fam}/{name}") ^ (seed * 0x9E3779B97F4A7C15)) & ((1 << 63) - 1))


def _uniform(g, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=g, dtype=torch.float64)


def _apply(fam, name, arr, seed):
    g = _gen(name, fam, seed)
    w = torch.from_numpy(np.asarray(arr)).to(torch.float64)
    if fam == "zero":
        w = torch.zeros_like(w)
    elif fam == "common":       # W[n, :] += 2 std(W) z_n
        w = w + K['common'] * w.std() * torch.randn(w.shape[0], generator=g, dtype=torch.float64)[:, None]
    elif fam == "colscale":     # input column k times 8^u_k
        s = K['colbase'] ** _uniform(g, w.shape[1], -1, 1)
        w = w * (s / s.pow(2).mean().sqrt())[None, :]
    elif fam == "heavy":        # Student-t, 3 degrees of freedom: z / sqrt(chi2_3 / 3), at the original standard deviation
        z = torch.randn(4, w.numel(), generator=g, dtype=torch.float32)
        t3 = z[0] / torch.sqrt((z[1] * z[1] + z[2] * z[2] + z[3] * z[3]) / 3)
        w = (t3 * float(w.std() / t3.double().std())).reshape(w.shape)
    elif fam == "norms":
        if name == "style_encoder.log_scale":
            w = torch.full_like(w, -0.5)
        else:                   # +- 8^u, negative with probability 0.3
            n = w.numel()
            sign = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < K['neg'], -1.0, 1.0)
            w = (sign * K['normbase'] ** _uniform(g, n, -1, 1)).reshape(w.shape)
    elif fam == "mod":          # biases: scales over [-0.99, 4], shifts over +-3, gate pre-activations over +-5
        H = DS.HIDDEN
        lo, hi = K['scale']
        scale = lambda: lo + (hi - lo) * _uniform(g, H, 0, 1) ** K['scale_pow']
        shift = lambda: _uniform(g, H, -K['shift'], K['shift'])
        gate = lambda: _uniform(g, H, -K['gate'], K['gate'])
        if name.startswith("dit.norm_out"):    # [scale | shift]
            parts = [scale(), shift()]
        else:                                   # [sh_a sc_a g_a sh_m sc_m g_m]
            parts = [shift(), scale(), gate(), shift(), scale(), gate()]
        w = torch.cat(parts)
    return w.to(torch.float32).numpy()


class Family:
    """lazy {name: fp32 ndarray} view of a state dict under one family"""

    def __init__(self, sd, fam, seed):
        if fam != "synth" and fam not in FAMILIES:
            raise KeyError(fam)
        self.sd, self.fam, self.seed, self._made = sd, fam, seed, {}

    def __contains__(self, k):
        return k in self.sd

    def __iter__(self):
        return iter(self.sd)

    def keys(self):
        return self.sd.keys()

    def __getitem__(self, k):
        base = self.sd[k]
        if not changes(self.fam, k, base):
            return base
        if k not in self._made:
            self._made[k] = _apply(self.fam, k, base, self.seed)
        return self._made[k]

    def changed(self, names=None):
        """the names this family changes (of `names`, default all)"""
        return [k for k in (self.sd if names is None else names) if changes(self.fam, k, self.sd[k])]


def family(sd, name: str, seed: int) -> Family:
    return Family(sd, name, seed)


def stage_names(names):
    """the tensors the STAGE cases read: DiT blocks 0, 1 and 11, the first two blocks of each encoder and the norm weight of the third
    (the image blocks [0, 2) leave), and everything outside the block stacks' inner tensors (the modulation chain, embed, head, the
    encoders' ends, every block's cross K / V)"""
    keep = []
    for k in names:
        m = re.match(r"dit\.transformer_blocks\.(\d+)\.(.*)", k)
        if m:
            cross = m.group(2).startswith(("attn.to_k_ref", "attn.to_v_ref", "attn.to_k_text", "attn.to_v_text", "attn.k_norm_cross",
                                           "attn_norm.linear"))
            if cross or int(m.group(1)) in (0, 1, 11):
                keep.append(k)
            continue
        m = re.match(r"(style_encoder|phoneme_embedding)\.blocks\.(\d+)\.", k)
        if m and int(m.group(2)) > 1 and not k.endswith(".blocks.2.attention_norm.weight"):
            continue
        keep.append(k)
    return keep


class Lazy64(dict):
    """a {name: ndarray} mapping viewed as fp64 tensors, converted on first use"""

    def __init__(self, sd):
        super().__init__()
        self.sd = sd

    def __getitem__(self, k):
        if not dict.__contains__(self, k):
            dict.__setitem__(self, k, torch.from_numpy(np.asarray(self.sd[k])).to(torch.float64))
        return dict.__getitem__(self, k)

    def get(self, k, default=None):
        return self[k] if k in self.sd else default


_SD: Dict[str, object] = {}


def base_sd():
    if "sd" not in _SD:
        _SD["sd"] = synth_state_dict(dit_param_specs(), SEED)
    return _SD["sd"]


def weights(fam: str):
    """(the family's lazy fp32 dict, its fp64 view), one per family and session"""
    if fam not in _SD:
        f = family(base_sd(), fam, SEED)
        _SD[fam] = (f, Lazy64(f))
    return _SD[fam]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
BLOCK_SHAPE = (5, 37, 9, 11)
MASSIVE_UTT, MASSIVE_CH, MASSIVE_X = 2, (7, 533), 300.0


def massive(x):
    """channels 7 and 533 of one utterance's residual at 300 times the row spread"""
    x = x.clone()
    sp = x[MASSIVE_UTT].std(-1)
    for ch in MASSIVE_CH:
        x[MASSIVE_UTT, :, ch] = MASSIVE_X * sp
    return x


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case:
    """key: what identifies the reference (path-independent); kinds: metric name -> kind of BOUND; nblk: blocks behind an increment"""
    nblk = 0

    def errors(self, got, ref):
        raise NotImplementedError


class BlockCase(Case):
    """DiT blocks [l0, l1) at 5 x 37 x 9 x 11 ragged; rs: one modulation row (0) or one per utterance (1)"""
    kinds = {"utt": "utt", "row": "row", "image": "row"}

    def __init__(self, rs, l0, l1, massive_in=False):
        self.rs, self.l0, self.l1, self.massive, self.nblk = rs, l0, l1, massive_in, l1 - l0
        self.key = ("blocks", rs, l0, l1, massive_in)
        B, N, R, P = BLOCK_SHAPE
        g = torch.Generator().manual_seed(B * 1000 + N + l0 + 7 * rs)
        self.x, self.mask, self.c = _inputs(B, N, R, P, g, True)
        if massive_in:
            self.x = massive(self.x)
        self.t = torch.rand(B if rs else 1, generator=g, dtype=torch.float64)
        self._tables = {}

    def plain(self):
        return case("blocks", self.rs, self.l0, self.l1, False)

    def table(self, w):
        """the modulation table the stage is GIVEN (fp32, from exact fp64: the stand-in reads the same one)"""
        if id(w) not in self._tables:
            with torch.no_grad(), DS.Rounding.off():
                self._tables[id(w)] = DS.mod_table(w, self.t).float()
        return self._tables[id(w)]

    def outputs(self, w, slip=None, table=None):
        B = self.x.shape[0]
        rows = DS.mod_rows(self.table(w) if table is None else table, B, 0, self.rs)
        x = self.x.double()
        for l in range(self.l0, self.l1):
            x = DS.dit_block(w, l, x, self.mask, rows, self.c, slip=slip)
        return {"x": x, "img": DS.next_image(x, rows, self.l1), "rows": rows}

    def errors(self, got, ref, img_ref=None):
        base = self.x.double()
        return {"utt": _rel_utt(got["x"], ref["x"], base), "row": _rel_rows(got["x"], ref["x"], base),
                "image": _rel_rows(got["img"], ref["img"] if img_ref is None else img_ref)}

    def floors(self, ref):
        base = self.x.double()
        return {"utt": 2 * self.nblk * _floor(ref["x"], base, _rel_utt), "row": 2 * self.nblk * _floor(ref["x"], base, _rel_rows)}


class EncBlockCase(Case):
    kinds = {"utt": "utt", "row": "row", "image": "row"}

    def __init__(self, net):
        self.net, self.l0, self.l1, self.nblk = net, 0, 2, 2
        self.key = ("enc blocks", net)
        self.S = 9 if net == "style" else 11
        g = torch.Generator().manual_seed(80 + self.S)
        self.km = _mask(_lengths(5, self.S, g), self.S)
        x = torch.randn(5, self.S, 512, generator=g, dtype=torch.float64)
        x[0] += 100.0 * x[0].std()
        self.x = x.float()

    def plain(self):
        return self

    def outputs(self, w, slip=None):
        x = self.x.double()
        for l in range(self.l0, self.l1):
            x = DS.enc_block(w, self.net, l, x, self.km)
        return {"x": x, "img": DS.enc_image(w, self.net, x, self.l1)}

    errors = BlockCase.errors
    floors = BlockCase.floors


class EncEndCase(Case):
    """the output projection on a final-norm image, then the cross K / V of all 12 blocks on its result"""
    kinds = {"out": "kv", "k": "kv", "v": "kv"}

    def __init__(self, net):
        self.net = net
        self.key = ("enc end", net)
        self.S = 9 if net == "style" else 11
        g = torch.Generator().manual_seed(90 + self.S)
        self.km = _mask(_lengths(5, self.S, g), self.S)
        self.x = torch.randn(5, self.S, 512, generator=g, dtype=torch.float64)

    def plain(self):
        return self

    def image(self, w):
        """the stage's input: the final norm's image of a seeded residual (it depends on the family's norm weight)"""
        return DS.enc_image(w, self.net, self.x, DS.ENC[self.net]["layers"]).float()

    def outputs(self, w, slip=None):
        out = DS.enc_out(w, self.net, self.image(w).double(), self.km)
        with DS.Rounding.off():   # the K / V stage reads the fp32 sequence of the exact output, under the stand-in too
            seq = DS.enc_out(w, self.net, self.image(w).double(), self.km).float()
        k, v = DS.cross_kv(w, self.net, seq.double(), knorm_name="k_norm" if slip == "k_norm_self" else "k_norm_cross")
        return {"out": out, "k": k, "v": v, "seq": seq}

    def errors(self, got, ref):
        rows = lambda z: z.transpose(2, 3).reshape(z.shape[0], z.shape[1], z.shape[3], -1)   # (12, B, S, 960)
        return {"out": _rel_rows(got["out"], ref["out"])[self.km.reshape(-1)],
                "k": _rel_rows(rows(got["k"]), rows(ref["k"])), "v": _rel_rows(rows(got["v"]), rows(ref["v"]))}

    def floors(self, ref):
        return {}


class CondCase(Case):
    """mod (the table from t), embed, head"""
    kinds = {"mod": "lin", "embed": "lin", "head": "lin"}
    key = ("cond",)

    def __init__(self):
        g = torch.Generator().manual_seed(70)
        self.t = torch.tensor([0.0, 1e-3, 0.5, 1.0, 0.25])
        B, N = 5, 37
        self.x_t = torch.randn(B, N, 64, generator=g)
        self.mask = _mask(_lengths(B, N, g), N)
        self.img = (DS.layer_norm(torch.randn(B, N, 960, generator=g, dtype=torch.float64)) * 1.3 + 0.1).float()

    def plain(self):
        return self

    def outputs(self, w, slip=None):
        return {"mod": DS.mod_table(w, self.t.double(), tanh_gates=slip != "no_tanh"), "embed": DS.embed(w, self.x_t.double(), self.mask),
                "head": DS.head(w, self.img.double(), col_shift=int(slip == "head_col_shift"))}

    def errors(self, got, ref):
        return {k: _rel_rows(got[k], ref[k]) for k in ("mod", "embed", "head")}

    def floors(self, ref):
        return {}


class WholeCase(Case):
    """cond_encode + one denoise_step at 3 x 13 x 5 x 7 ragged, per utterance (TOL of tests/test_dit_gpu.py, bf16x3)"""
    kinds = {"velocity": None}
    key = ("whole",)

    def __init__(self):
        g = torch.Generator().manual_seed(60)
        B, N, R, P = 3, 13, 5, 7
        self.ref = torch.randn(B, R, 64, generator=g)
        self.ref_len = torch.tensor([R, 1, 3])
        self.ids = torch.randint(1, 198, (B, P), generator=g)
        self.pm = _mask(torch.tensor([P, 2, 5]), P)
        self.mask = _mask(torch.tensor([N, 1, 8]), N)
        self.x_t = torch.randn(B, N, 64, generator=g)
        self.t = torch.tensor([0.1, 0.5, 0.9])

    def plain(self):
        return self

    def outputs(self, w, slip=None):
        with torch.no_grad():
            c = DS.encode_conditions(w, self.ref, self.ref_len, self.ids, self.pm)
            return {"velocity": DS.denoise_step(w, self.x_t, self.mask, self.t, c, self.pm)}

    def errors(self, got, ref):
        m = self.mask[..., None].double()   # frames outside the mask are not part of the operator's contract
        return {"velocity": _rel_utt(got["velocity"].double().cpu() * m, ref["velocity"] * m)}

    def floors(self, ref):
        return {}


_CASES: Dict[tuple, Case] = {}
_KINDS = {"blocks": BlockCase, "enc blocks": EncBlockCase, "enc end": EncEndCase, "cond": CondCase, "whole": WholeCase}


def case(kind, *args) -> Case:
    """one Case per (kind, arguments) and session: its inputs are seeded, its references are kept by its key"""
    if (kind, *args) not in _CASES:
        _CASES[(kind, *args)] = _KINDS[kind](*args)
    return _CASES[(kind, *args)]


# what the GPU test runs: (modulation rows, path, presets) x block ranges; the encoders' paths x presets
BLOCK_RUNS = [(0, "fold", ("bf16x3", "f16", "bf16")), (1, "splitk", ("bf16x3", "f16")), (1, "unsplit", ("bf16x3", "f16"))]
BLOCK_RANGES = [(0, 2), (11, 12)]
ENC_RUNS = [(path, prec) for path in ("fold", "splitk") for prec in ("bf16x3", "f16")]
PRESETS = ("bf16x3", "f16", "bf16")
MASSIVE_FAMILIES = ("synth", "common", "mod")


def bounded_cases(fam):
    """every (case, preset) whose outputs the GPU test bounds by BOUND x A under `fam` (paths share a reference)"""
    out = []
    if fam in MASSIVE_FAMILIES:
        out += [(case("blocks", rs, l0, l1, True), p) for rs, p in _rs_presets() for l0, l1 in BLOCK_RANGES]
    if fam in FAMILIES and fam != "zero":
        out += [(case("blocks", rs, l0, l1, False), p) for rs, p in _rs_presets() for l0, l1 in BLOCK_RANGES]
        out += [(case(kind, net), p) for kind in ("enc blocks", "enc end") for net in ("style", "text") for p in ("bf16x3", "f16")]
        out += [(case("cond"), p) for p in PRESETS]
        out += [(case("whole"), "bf16x3")]
    return out


def _rs_presets():
    seen = []
    for rs, _, precs in BLOCK_RUNS:
        seen += [(rs, p) for p in precs if (rs, p) not in seen]
    return seen


# ---- the stand-in's error and A ---------------------------------------------------------------------------------------------
_REF: Dict[tuple, dict] = {}     # (family, case key) -> exact outputs
_EMODEL: Dict[tuple, tuple] = {}  # (family, case key, preset) -> ({metric: errors}, amax per site)


def exact(fam, case):
    k = (fam, case.key)
    if k not in _REF:
        with torch.no_grad():
            _REF[k] = case.outputs(weights(fam)[1])
    return _REF[k]


def e_model(fam, case, preset):
    """the stand-in's error per metric against exact fp64, and the largest |operand| each site saw"""
    k = (fam, case.key, preset)
    if k not in _EMODEL:
        w = weights(fam)[1]
        with torch.no_grad(), DS.Rounding(preset) as r:
            got = case.outputs(w)
        _EMODEL[k] = (case.errors(got, exact(fam, case)), dict(r.amax), got)
    return _EMODEL[k]


def amplification(fam, case, preset):
    """{metric: A per row / utterance} = max(1, e_model / e0), e0 the largest e_model of the same case under the shipped synthetic
    weights and the plain inputs"""
    e = e_model(fam, case, preset)[0]
    e0 = e_model("synth", case.plain(), preset)[0]
    return {m: (e[m] / e0[m].max()).clamp_min(1.0) for m in e}


def allowance(fam, case, preset, bound=None):
    """{metric: allowance per row / utterance} = BOUND[(kind, preset)] x A (+ the fp32 storage floor of block increments)"""
    A = amplification(fam, case, preset)
    fl = case.floors(exact(fam, case))
    out = {}
    for m, a in A.items():
        b = BOUND[(case.kinds[m], preset)] if bound is None else bound
        out[m] = b * a + fl.get(m, 0.0)
    return out, A
