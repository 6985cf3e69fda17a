"""Weight families and inputs that put every stage of the two latent scorers in its live range (tests/test_scorer_stages_gpu.py,
tests/test_scorer_stages_cpu.py).  Test infrastructure: numpy / torch only, no GPU.

They are STRUCTURED SYNTHETIC WEIGHTS, NOT A TRAINED MODEL.  A trained checkpoint is not at hand; under weights.init_rule alone the
verifier's activations grow through the blocks until its squeeze-excite gates are switches, four MFA channels in ten are constant over
time and the attentive pooling is a plain mean, and the recogniser's attention is never peaked and its output never confident.  Every
family starts from synth_state_dict(seed) and is seeded and lazy: state(net, family) is built on first use and kept.

Verifier
  "calibrated"         every BatchNorm's running_mean / running_var <- the statistics of one batch: one pass of the fp64 restatement in
                       training mode with momentum 1.0 over CALIB_BATCH = 8 x 60 seeded randn frames.  Nothing else changes.
  "calibrated+peaked"  the same, and asp.conv.weight times PEAK_SCALE, so that the pooling's softmax picks frames.
  SV_CONDITIONS (asserted from the reference alone, tests/test_scorer_stages_cpu.py): at most 5 % of the attention's tanh arguments
  beyond +-3; every squeeze-excite gate inside (0.05, 0.95); no MFA channel constant over time; under "calibrated+peaked" the largest
  pooling weight has a median over channels of at least 0.3 at n = 40.
Recogniser
  "peaked"   the q and k rows of every in_proj_weight times QK_SCALE and proj.weight times PROJ_SCALE: the largest attention weight has a
             median over (frame, head) of at least 0.5 in at least four of the seven layers, and at least half of the frames have a
             top-class probability of at least 0.9.
  "norms"    every LayerNorm weight +- 10^u, u uniform in [-1, 1], negative with probability 0.3; the conv module's BatchNorm running_var
             log-uniform in [0.01, 1].
The conditions are conditions of the weights on plain randn latents; the other inputs below are there to leave the live range.
Inputs (both scorers): randn latents; the same times 30; a row whose frames are all identical (zero variance over time: the verifier's
uniform and weighted std and its squeeze mean); a row with one frame whose 64 channels are equal (the recogniser's LayerNorm variance 0)."""
import functools

import torch

from smalltts_amd.weights import fnv1a64
from tests.helpers import asr_ref, sv_ref

SEED = 5
SV_FAMILIES = ("synth", "calibrated", "calibrated+peaked")
ASR_FAMILIES = ("synth", "peaked", "norms")
CALIB_BATCH = (8, 60)
# asp.conv.weight: at n = 40 the reference's median largest pooling weight is 0.65 at 8, 0.91 at 16, 0.98 at 24, 0.994 at 32
PEAK_SCALE = 16.0
# at (2, 8) the attention medians are 0.14 .. 0.46 and a quarter of the frames confident; at (3, 12) 0.47 .. 0.79 and 0.41 .. 0.49; at
# (3, 24) the same medians and 0.69 .. 0.77 of the frames; at (4, 16) the attention is nearly one-hot (0.85 .. 0.95)
QK_SCALE, PROJ_SCALE = 3.0, 24.0
SV_CONDITIONS = dict(tanh_beyond_3=0.05, gate_lo=0.05, gate_hi=0.95, peak_median=0.3)
ASR_CONDITIONS = dict(attn_median=0.5, attn_layers=4, confident=0.9, confident_frames=0.5)
INPUT_KINDS = ("randn", "x30", "const_row", "flat_frame")
# (input kind, B, N, lengths): ragged batches at the smallest lengths that cross every tile edge.
# Verifier: 6 the minimum (the d = 5 reflect touches both ends), 7, 32 / 33 the res2net blocks of 32 frames, 64 / 65 sv_tdnn's tile,
# 129 ten res2net blocks (two waves take two each), 225 the longest; a row under 6 frames has the zero embedding.
SV_CASES = [("randn", 3, 7, [7, 6, 3]), ("randn", 2, 33, [33, 32]), ("randn", 2, 65, [65, 64]), ("randn", 1, 129, [129]),
            ("randn", 1, 225, [225]), ("x30", 2, 40, [40, 33]), ("const_row", 2, 40, [40, 33]), ("flat_frame", 2, 40, [40, 33])]
# Recogniser (T = 4 N frames): 1; 14 / 15 the conv tile of 56 and a second tile that holds halo-fed frames only; 16 / 17 the 64-frame
# tile; 29 (T = 2 x 56 + 4); 64 / 65 the attention's 256-query block; 225 (T = 900, the attention's limit).
ASR_CASES = [("randn", 3, 15, [15, 14, 1]), ("randn", 2, 17, [17, 16]), ("randn", 1, 29, [29]), ("randn", 2, 65, [65, 64]),
             ("randn", 1, 225, [225]), ("x30", 2, 29, [29, 16]), ("const_row", 2, 29, [29, 16]), ("flat_frame", 2, 29, [29, 16])]
CASES = {"sv": SV_CASES, "asr": ASR_CASES}


def case_id(c):
    return f"{c[0]}-{c[2]}-" + "_".join(str(n) for n in c[3])


def _gen(tag):
    return torch.Generator().manual_seed(fnv1a64(f"scorer_families/{tag}") & ((1 << 63) - 1))


@functools.lru_cache(maxsize=None)
def state(net: str, fam: str, seed: int = SEED):
    """{tensor name without the "sv." / "asr." prefix: float32 torch tensor} of a family"""
    if net == "sv":
        sd = sv_ref.state_dict(seed)
        if fam == "synth":
            return sd
        m = sv_ref.SVRef()
        m.load_state_dict(sd, strict=False)
        m = m.double().train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.momentum = 1.0
        with torch.no_grad():
            m(torch.randn(*CALIB_BATCH, 64, generator=_gen(f"calib/{seed}"), dtype=torch.float64))
        out = {k: v.float() for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")}
        if fam == "calibrated+peaked":
            out["ecapa.asp.conv.conv.weight"] = out["ecapa.asp.conv.conv.weight"] * PEAK_SCALE
        elif fam != "calibrated":
            raise KeyError(fam)
        return out
    sd = asr_ref.state_dict(seed)
    if fam == "synth":
        return sd
    out = dict(sd)
    for k, v in sd.items():
        g = _gen(f"{fam}/{k}/{seed}")
        if fam == "peaked":
            if k.endswith("in_proj_weight"):
                w = v.clone()
                w[:128] *= QK_SCALE
                out[k] = w
            elif k == "proj.weight":
                out[k] = v * PROJ_SCALE
        elif fam == "norms":
            if k.endswith("norm.weight") or k.endswith("sequential.0.weight") and v.dim() == 1:
                sign = torch.where(torch.rand(v.numel(), generator=g) < 0.3, -1.0, 1.0)
                out[k] = (sign * 10.0 ** (2 * torch.rand(v.numel(), generator=g) - 1)).float()
            elif k.endswith("running_var"):
                out[k] = (10.0 ** (-2 * torch.rand(v.numel(), generator=g))).float()
        else:
            raise KeyError(fam)
    return out


@functools.lru_cache(maxsize=None)
def model(net: str, fam: str, dtype=torch.float64, seed: int = SEED):
    """the restatement under a family, eval mode"""
    m = sv_ref.SVRef() if net == "sv" else asr_ref.ASRRef()
    missing, unexpected = m.load_state_dict(state(net, fam, seed), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


def engine_state(net: str, fam: str, seed: int = SEED):
    """{full tensor name: float32 ndarray}: what HipEngine.load_state_dict takes"""
    return {f"{net}.{k}": v.numpy() for k, v in state(net, fam, seed).items()}


def latents(kind: str, B: int, N: int, tag: str = ""):
    """(B, N, 64) float32 latents of one of INPUT_KINDS; the special row / frame sits in row 0"""
    x = torch.randn(B, N, 64, generator=_gen(f"latents/{tag}/{B}/{N}"))
    if kind == "x30":
        x = x * 30
    elif kind == "const_row":
        x[0] = x[0, 0]
    elif kind == "flat_frame":
        x[0, N // 2] = x[0, N // 2, 0]
    elif kind != "randn":
        raise KeyError(kind)
    return x
