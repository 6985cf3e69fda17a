"""GPU: every codec kernel path held to fp64, one stage at a time (smtts_test_codec_stage / HipEngine.test_codec_stage).

The whole-call tests (test_codec_gpu.py and friends) bound a decode by its audio SNR over ~20 blocks, and compare alternative paths
with each other bit for bit.  Here each stage of the finalized decoder / encoder runs alone through the product's own dispatch, at
frame counts where tiles, segments and halos line up badly, and is compared with the plain fp64 statement of that stage
(oracle/codec_stages.py, pinned to the CPU oracle by tests/test_codec_oracle.py) on the engine's own weights:
- blocks: the increment out - x against ref - x (the residual would hide a wrong branch), rel-L2 per utterance;
- resampling, stem and head: the output itself, rel-L2 per utterance;
the worst utterance is reported, so a quiet utterance is not averaged into a loud one.

Bounds: about twice the worst value measured on an MI355X (the measured value stands next to each), never above the ceilings
bf16x3 5e-5 (blocks) / 2e-5 (resampling, stem, head GEMMs), f16 2e-3, bf16 1.5e-2, f16x2 ConvTranspose 1e-3."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

from oracle import codec_stages as CS
from oracle.dit_oracle import to_torch
from smalltts_amd.weights import CodecSpec, codec_decoder_param_specs, codec_encoder_param_specs, synth_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11

SPECS = {
    # the default widths (C = 2048 ... 32) with one block per stage: every wide-stage path at few parameters
    "wide": CodecSpec(n_filters=32, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1)),
    # C = 64 / 32 with two / three blocks.  The encoder mirrors the decoder (enc_depths = reversed(dec_depths)), so the C = 32 stage
    # has the same depth on both sides: the stage chain with nb = 3 here, nb = 2 in "c32d2".  A single block never takes the chain
    # in the shipped build (Engine::chain_min_blocks_ = 2)
    "c32": CodecSpec(n_filters=32, ratios=(2,), dec_depths=(2, 3)),
    "c32d2": CodecSpec(n_filters=32, ratios=(2,), dec_depths=(1, 2)),
    # k = 5: the k = 7-only kernels (block / chain wave, mixer_wide, streaming mixer) step aside
    "k5": CodecSpec(n_filters=64, ratios=(2, 2, 2, 2), dec_depths=(1, 1, 1, 1, 1), kernel=5),
    # F % 64 != 0 (C = 8, F = 32): the all-fp32 hidden path
    "tiny": CodecSpec(n_filters=8, ratios=(4, 2, 2), dec_depths=(2, 1, 1, 2)),
    # absent biases and layer scales, a final norm in front of both heads
    "bare": CodecSpec(n_filters=32, ratios=(2, 2), dec_depths=(1, 1, 1), conv_bias=False, ffn_bias=False, layer_scale=False,
                      final_norm=True),
}

# bound per (kind, precision): kind "blk" = blocks (their increment when run alone), "lin" = resampling / stem / head.  About twice the
# worst case measured on an MI355X over the table below, which stands in the comment.
BOUND = {
    ("blk", "bf16x3"): 2.5e-5,   # measured 1.04e-5 (demoted blocks, w1 rows x 30000), 6.95e-6 otherwise (64x64 split-K, C = 2048)
    ("lin", "bf16x3"): 1e-5,     # measured 4.95e-6 (decoder stem)
    ("blk", "f16"): 1.4e-3,      # measured 6.70e-4 (w1 rows x 300: pre-activations of several hundred), 5.45e-4 otherwise (C = 32, T = 2)
    ("lin", "f16"): 1e-5,        # the f16 preset keeps the resampling / stem / head site split-bf16: measured 4.95e-6
    ("blk", "bf16"): 1.2e-2,     # measured 5.93e-3 (stage chain, encoder)
    ("lin", "bf16"): 5e-3,       # measured 2.41e-3 (ConvTranspose K = 2048 on gemm3)
    ("lin", "f16,codec_conv=f16x2"): 4.5e-4,   # measured 2.14e-4 (ConvTranspose K = 1024)
}
MEASURED = {}   # (case id) -> worst error: printed at the end of the run
SEEN = set()    # kernel classes the cases launched (profiler names)


class _Lazy64(dict):
    """fp32 state dict viewed as fp64 tensors, converted on first use (the wide spec holds 86 M parameters per half)."""

    def __init__(self, sd):
        super().__init__()
        self.sd = sd

    def __getitem__(self, k):
        if not dict.__contains__(self, k):
            dict.__setitem__(self, k, torch.from_numpy(np.asarray(self.sd[k])).to(torch.float64))
        return dict.__getitem__(self, k)

    def get(self, k, default=None):
        return self[k] if k in self.sd else default


_SD = {}
_ENG = {}


def _sd(spec_name, part, seed=SEED):
    key = (spec_name, part, seed)
    if key not in _SD:
        specs = (codec_decoder_param_specs if part == "decoder" else codec_encoder_param_specs)(SPECS[spec_name])
        _SD[key] = synth_state_dict(specs, seed)
    return _SD[key]


def _engine(spec_name, env=(), sd=None):
    """One engine per (spec, environment switches); switches are read when the engine is created."""
    from smalltts_amd.engine import HipEngine
    key = (spec_name, env, id(sd))
    if sd is None and key in _ENG:
        return _ENG[key]
    old = {k: os.environ.get(k) for k, _ in env}
    os.environ.update(dict(env))
    try:
        eng = HipEngine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    spec = SPECS[spec_name]
    if sd is None:
        eng.load_synthetic(SEED, parts=("decoder", "encoder"), codec_spec=spec)
    else:
        eng.set_codec_spec(spec)
        eng.load_state_dict(sd)
    eng.finalize()
    if sd is None:
        _ENG[key] = eng
    return eng


def _in_dims(spec, part, stage, what):
    """C_in of the hook's input"""
    dec = part == "decoder"
    chans = [spec.dec_channels(i) for i in range(spec.n_stages)]
    if not dec:
        chans = chans[::-1]
    if what & 1:
        return (spec.latent_dim if dec else 1)
    if what & 2:
        return chans[stage - 1]
    return chans[stage]


def _inputs(B, T, C, g, edge="plain"):
    """B utterances of T frames, different contents.  edge: "plain"; "silence" (utterance 1 all zero); "scales" (utterance 0 x 1e3,
    utterance 2 x 1e-3); "spikes" (isolated loud frames at tile / segment boundaries)."""
    x = torch.randn(B, T, C, generator=g, dtype=torch.float64)
    x = x * (1.0 + torch.arange(B, dtype=torch.float64)[:, None, None])   # utterances of different loudness
    if edge == "silence" and B > 1:
        x[1] = 0
    elif edge == "scales" and B > 2:
        x[0] *= 1e3
        x[2] *= 1e-3
    elif edge == "spikes":
        for t in (0, 31, 32, 41, 42, 43, 84):
            if t < T:
                x[:, t] *= 50.0
    return x


def _per_utt(got, ref, base=None):
    """[(rel-L2 of got - ref, fp32 storage floor of ref)] per utterance, both relative to the utterance's own reference (its
    increment when base is given).  An all-zero reference must come out exactly zero and gives (0, 0)."""
    got, ref = got.to(torch.float64), ref.to(torch.float64)
    out = []
    for b in range(ref.shape[0]):
        d = ref[b] - (base[b] if base is not None else 0)
        nd = float(d.norm())
        if nd == 0.0:
            assert float((got[b] - ref[b]).norm()) == 0.0
            out.append((0.0, 0.0))
            continue
        out.append((float((got[b] - ref[b]).norm()) / nd, float((ref[b].float().double() - ref[b]).norm()) / nd))
    return out


def _assert_within(case_id, per_utt, bound):
    """Each utterance against the bound plus twice its OWN fp32 storage floor: the stored output is fp32, so a loud utterance's
    increment cannot come closer to fp64 than the rounding of x + increment itself, and that allowance is not lent to its neighbours."""
    MEASURED[case_id] = (max(e for e, _ in per_utt), bound)
    for b, (e, f) in enumerate(per_utt):
        assert e <= bound + 2 * f, f"{case_id}: utterance {b} rel err {e:.3e} > {bound:.1e} (its fp32 floor {f:.1e})"


def _run_hook(eng, part, stage, what, x):
    """runs the hook with the profiler on; returns (output on the host, names of the kernel classes it launched)"""
    eng.profile(True)
    try:
        out = eng.test_codec_stage(part, stage, what, x.float())
        torch.cuda.synchronize()
        names = {k["name"] for k in eng.profile_report()}
    finally:
        eng.profile(False)
    SEEN.update(names)
    return out.cpu(), names


def _check(case_id, eng, spec_name, part, stage, what, x, prec, sd=None, repeat=True):
    spec = SPECS[spec_name]
    w = _Lazy64(sd if sd is not None else _sd(spec_name, part))
    got, names = _run_hook(eng, part, stage, what, x)
    if repeat:   # two runs of the hook give the same bits
        assert torch.equal(eng.test_codec_stage(part, stage, what, x.float()).cpu(), got), f"{case_id}: not repeatable"
    xin = x.float().double()   # the kernel sees the fp32 input
    with torch.no_grad():
        ref = CS.stage(w, part, stage, what, xin, spec)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), case_id
    # blocks alone: their increment; anything else (or blocks with the resampling / head around them): the output itself, at the
    # block bound when blocks are part of it
    _assert_within(case_id, _per_utt(got, ref, xin if what == 4 else None), BOUND[("blk" if what & 4 else "lin", prec)])
    return got, names


# ---- the case table ----------------------------------------------------------------------------------------------------------
# (spec, part, stage, what, B, T, precision, edge, fused, env, tuning) -- what: 1 stem, 2 resampling, 4 blocks, 8 head
W, D, E = "wide", "decoder", "encoder"
CASES = {
    # decoder stem (fp32-A GEMM over K * latent) and the ConvTranspose paths
    "dec_stem": ("wide", D, 0, 1, 3, 7, "bf16x3", "scales", True, (), None),
    "dec_stem_f16": ("wide", D, 0, 1, 1, 1, "f16", "plain", True, (), None),
    "dec_up1_g3split": ("wide", D, 1, 2, 3, 2, "f16", "silence", True, (), None),            # K = 4096: gemm3 on the split image
    "dec_up2_g3split_bf16": ("wide", D, 2, 2, 1, 6, "bf16", "plain", True, (), None),         # K = 2048
    "dec_up3_fp32a": ("wide", D, 3, 2, 3, 7, "bf16x3", "spikes", True, (), None),            # K = 1024: fp32-A kernel
    "dec_up3_f16x2": ("wide", D, 3, 2, 3, 7, "f16,codec_conv=f16x2", "plain", True, (), None),
    "dec_up4_f16x2": ("wide", D, 4, 2, 3, 31, "f16,codec_conv=f16x2", "scales", True, (), None),   # K = 512
    "dec_up5_wave": ("wide", D, 5, 2, 3, 33, "bf16x3", "spikes", True, (), None),             # codec_upsample_wave<256x128>
    "dec_up6_wave": ("wide", D, 6, 2, 1, 85, "f16", "plain", True, (), None),                 # <128x64>
    "dec_up1_unfused": ("wide", D, 1, 2, 1, 2, "bf16x3", "plain", False, (), None),           # fp32-A at K = 4096
    # decoder blocks by width
    "dec_s0_t160_splitk": ("wide", D, 0, 4, 1, 600, "f16", "plain", True, (), None),          # M = 600: 160x128 split-K
    "dec_s0_64x64_splitk": ("wide", D, 0, 4, 3, 41, "bf16x3", "silence", True, (), None),     # M = 123: 64x64 split-K
    "dec_s0_bf16": ("wide", D, 0, 4, 3, 7, "bf16", "scales", True, (), None),
    "dec_s0_unsplit": ("wide", D, 0, 4, 1, 700, "f16", "plain", True, (), None),              # M = 700: one gemm3 resid
    "dec_s1_mixer_wide": ("wide", D, 1, 4, 3, 43, "bf16x3", "spikes", True, (), None),
    "dec_s2_mixer_wide_f16": ("wide", D, 2, 4, 3, 31, "f16", "scales", True, (), None),
    "dec_s2_two_kernel_mixer": ("wide", D, 2, 4, 3, 33, "bf16x3", "plain", True, (("SMTTS_MIXER_WIDE", "0"),), None),
    "dec_s3_stream256": ("wide", D, 3, 4, 3, 85, "bf16x3", "spikes", True, (), None),         # segments of 42: 42 + 42 + 1
    "dec_s3_stream256_f16": ("wide", D, 3, 4, 1, 43, "f16", "plain", True, (), None),
    "dec_s4_stream128": ("wide", D, 4, 4, 3, 41, "f16", "silence", True, (), None),
    "dec_s4_stream128_bf16": ("wide", D, 4, 4, 3, 6, "bf16", "plain", True, (), None),
    "dec_s5_block_wave64": ("wide", D, 5, 4, 3, 64, "f16", "spikes", True, (), None),
    "dec_s5_mixer_ffn_wave64": ("wide", D, 5, 4, 3, 43, "f16", "scales", True, (), None),     # T % 32 != 0
    "dec_s5_bf16x3": ("wide", D, 5, 4, 1, 64, "bf16x3", "plain", True, (), None),             # C = 64 at bf16x3: no block wave
    "dec_s6_block_wave32": ("wide", D, 6, 4, 3, 1056, "f16", "spikes", True, (), None),
    "dec_s6_block_wave32_bf16x3": ("wide", D, 6, 4, 1, 32, "bf16x3", "plain", True, (), None),
    "dec_s6_ffn_wave32": ("wide", D, 6, 4, 3, 33, "bf16x3", "silence", True, (), None),
    "dec_s6_t2": ("wide", D, 6, 4, 3, 2, "f16", "plain", True, (), None),
    "dec_s6_head": ("wide", D, 6, 8, 3, 85, "bf16x3", "scales", True, (), None),
    "dec_s6_head_long": ("wide", D, 6, 8, 1, 1056, "f16", "spikes", True, (), None),          # head_conv32 (T >= 256)
    # unfused: rmsnorm + dwconv_resid, gemm3 pair / fp32-A hidden
    "dec_s3_unfused": ("wide", D, 3, 4, 3, 7, "bf16x3", "plain", False, (), None),
    "dec_s6_unfused": ("wide", D, 6, 4, 3, 31, "bf16x3", "plain", False, (), None),
    "dec_s1_unfused_f16": ("wide", D, 1, 4, 1, 41, "f16", "plain", False, (), None),
    # encoder
    "enc_stem": ("wide", E, 0, 1, 3, 85, "bf16x3", "scales", True, (), None),
    "enc_down1": ("wide", E, 1, 2, 3, 86, "bf16x3", "spikes", True, (), None),                # K = 128: fp32-A
    "enc_down3_fp32a": ("wide", E, 3, 2, 3, 28, "f16", "plain", True, (), None),             # K = 1024
    "enc_down4_smallm": ("wide", E, 4, 2, 3, 35, "bf16x3", "silence", True, (), None),        # K = 2560: split-K gemm3
    "enc_down6_smallm": ("wide", E, 6, 2, 1, 48, "bf16x3", "plain", True, (), None),          # K = 16384
    "enc_down6_smallm_bf16": ("wide", E, 6, 2, 3, 16, "bf16", "scales", True, (), None),
    "enc_down5_fp32a_unfused": ("wide", E, 5, 2, 1, 35, "bf16x3", "plain", False, (), None),
    "enc_head_smallm": ("wide", E, 6, 8, 3, 7, "bf16x3", "scales", True, (), None),           # K = 14336
    "enc_head_fp32a": ("wide", E, 6, 8, 3, 6, "f16", "plain", False, (), None),
    "enc_down2": ("wide", E, 2, 2, 3, 42, "f16", "plain", True, (), None),                    # K = 256: fp32-A
    "enc_down5_smallm": ("wide", E, 5, 2, 3, 25, "bf16x3", "scales", True, (), None),          # K = 5120: split-K gemm3
    "enc_s0_blocks": ("wide", E, 0, 4, 3, 33, "f16", "spikes", True, (), None),
    "enc_s1_blocks": ("wide", E, 1, 4, 3, 43, "bf16x3", "plain", True, (), None),
    "enc_s2_blocks": ("wide", E, 2, 4, 3, 41, "f16", "silence", True, (), None),
    "enc_s3_blocks": ("wide", E, 3, 4, 3, 85, "bf16x3", "spikes", True, (), None),
    "enc_s4_blocks": ("wide", E, 4, 4, 3, 31, "f16", "scales", True, (), None),
    "enc_s5_blocks": ("wide", E, 5, 4, 3, 7, "bf16x3", "plain", True, (), None),
    "enc_s6_blocks": ("wide", E, 6, 4, 1, 2, "f16", "plain", True, (), None),
    # the stage chain (all blocks of a C = 32 stage in one launch), both tunings; throughput: runs start inside utterances
    "chain3_latency": ("c32", D, 1, 4, 3, 1056, "f16", "spikes", True, (("SMTTS_STAGE_CHAIN", "2"),), "latency"),
    "chain3_throughput": ("c32", D, 1, 4, 3, 1056, "f16", "plain", True, (("SMTTS_STAGE_CHAIN", "2"),), "throughput"),
    "chain3_encoder": ("c32", E, 0, 4, 3, 96, "bf16", "silence", True, (("SMTTS_STAGE_CHAIN", "2"),), "throughput"),
    "chain2_latency": ("c32d2", D, 1, 4, 3, 1056, "f16", "spikes", True, (("SMTTS_STAGE_CHAIN", "2"),), "latency"),
    "chain2_throughput_bf16": ("c32d2", D, 1, 4, 3, 1056, "bf16", "plain", True, (("SMTTS_STAGE_CHAIN", "2"),), "throughput"),
    "chain2_encoder": ("c32d2", E, 0, 4, 3, 96, "f16", "silence", True, (("SMTTS_STAGE_CHAIN", "2"),), "throughput"),
    "c32_depth2_c64": ("c32", D, 0, 4, 3, 33, "bf16x3", "plain", True, (), None),
    # k = 5: the fallbacks of the k = 7-only kernels
    "k5_c1024_dwconv_rms": ("k5", D, 0, 4, 3, 7, "bf16x3", "plain", True, (), None),
    "k5_c512": ("k5", D, 1, 2 | 4, 3, 6, "f16", "spikes", True, (), None),
    "k5_c128_staged_mixer": ("k5", D, 3, 4, 3, 43, "bf16x3", "plain", True, (), None),
    "k5_c64": ("k5", D, 4, 4, 3, 64, "f16", "plain", True, (), None),
    "k5_head": ("k5", D, 4, 8, 3, 6, "bf16x3", "plain", True, (), None),
    "k5_enc_stem": ("k5", E, 0, 1, 1, 31, "bf16x3", "plain", True, (), None),
    # F % 64 != 0, final norm / no biases / no layer scales
    "tiny_c8_fp32_hidden": ("tiny", D, 3, 4, 3, 41, "bf16x3", "plain", True, (), None),
    "tiny_c8_f16": ("tiny", D, 3, 2 | 4 | 8, 3, 7, "f16", "plain", True, (), None),
    "bare_dec_head_final_norm": ("bare", D, 2, 4 | 8, 3, 43, "bf16x3", "scales", True, (), None),
    "bare_enc_head_final_norm": ("bare", E, 2, 8, 3, 7, "bf16x3", "plain", True, (), None),
    "bare_dec_stem": ("bare", D, 0, 1, 3, 6, "bf16x3", "plain", True, (), None),
}


@pytest.mark.parametrize("case", list(CASES))
def test_stage_vs_fp64(case):
    spec_name, part, stage, what, B, T, prec, edge, fused, env, tuning = CASES[case]
    spec = SPECS[spec_name]
    eng = _engine(spec_name, env)
    eng.set_precision(prec)
    if tuning:
        eng.set_tuning(tuning)
    eng.lib.smtts_test_set_fused_ffn(eng.h, int(fused))
    try:
        C = _in_dims(spec, part, stage, what)
        g = torch.Generator().manual_seed(zlib.crc32(case.encode()))
        x = _inputs(B, T, C, g, edge)
        if what & 1 and part == E:
            x = x * 0.3
        _, names = _check(case, eng, spec_name, part, stage, what, x, prec)
        if "codec_chain_wave<32>" in names:   # the chain is one template per block count (its LDS layout depends on it)
            depth = (spec.dec_depths if part == D else tuple(reversed(spec.dec_depths)))[stage]
            SEEN.add(f"codec_chain_wave<32> nb={depth}")
    finally:
        eng.lib.smtts_test_set_fused_ffn(eng.h, 1)
        if tuning:
            eng.set_tuning("latency")


_CHILD = r"""
import sys, json, numpy as np, torch
sys.path.insert(0, sys.argv[3])
from smalltts_amd.engine import HipEngine
from smalltts_amd.weights import CodecSpec
spec = CodecSpec(n_filters=32, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))
eng = HipEngine(0, "bf16x3")
eng.load_synthetic(int(sys.argv[2]), parts=("decoder",), codec_spec=spec)
eng.finalize()
x = torch.from_numpy(np.load(sys.argv[1] + ".in.npy"))
eng.profile(True)
outs = [eng.test_codec_stage("decoder", s, 4, x[..., : spec.dec_channels(s)].contiguous()).cpu().numpy() for s in (3, 4)]
names = [k["name"] for k in eng.profile_report()]
np.savez(sys.argv[1] + ".out.npz", s3=outs[0], s4=outs[1])
json.dump(names, open(sys.argv[1] + ".names.json", "w"))
"""


@pytest.mark.parametrize("stream", ["122", "0"])
def test_mixer_segment_lengths_and_staged_mixer_vs_fp64(tmp_path, stream):
    """launch_mixer_fused reads SMTTS_MIXER_STREAM once per process: segments of 122 frames and the LDS-staged kernel (0) run in a child
    process each, on the C = 256 / 128 stages, with utterance ends inside segments and tiles."""
    import json
    spec = SPECS["wide"]
    g = torch.Generator().manual_seed(7)
    x = _inputs(3, 130, 256, g, "spikes")
    base = str(tmp_path / f"mix{stream}")
    np.save(base + ".in.npy", x.float().numpy())
    env = dict(os.environ, SMTTS_MIXER_STREAM=stream)
    subprocess.run([sys.executable, "-c", _CHILD, base, str(SEED), ROOT], check=True, env=env, timeout=300)
    got = np.load(base + ".out.npz")
    SEEN.update(json.load(open(base + ".names.json")))
    w = _Lazy64(_sd("wide", D))
    for s, key in ((3, "s3"), (4, "s4")):
        xin = x[..., : spec.dec_channels(s)].float().double()
        with torch.no_grad():
            ref = CS.stage(w, D, s, 4, xin, spec)
        _assert_within(f"mixer_stream_{stream}_s{s}", _per_utt(torch.from_numpy(got[key]), ref, xin), BOUND[("blk", "bf16x3")])


def test_f16_ffn_far_from_the_origin_and_demoted_blocks():
    """ffn.w1 rows scaled until the C = 64 / 32 blocks' pre-activations reach several hundred while the fused kernels stay certified:
    finite, within the f16 bound (the packed GELU far from the origin).  A factor whose bound leaves the fp16 range demotes the
    block, which must then meet the bf16x3 bound."""
    import warnings
    spec_name = "c32"
    base = _sd(spec_name, D, 4)
    for factor, prec_bound, demoted in ((300.0, "f16", False), (30000.0, "bf16x3", True)):
        sd = dict(base)
        rng = np.random.default_rng(3)
        for k in [k for k in sd if k.endswith("ffn.w1.weight")]:
            rows = rng.choice(sd[k].shape[0], size=sd[k].shape[0] // 8, replace=False)
            sd[k] = sd[k].copy()
            sd[k][rows] *= np.float32(factor)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            eng = _engine(spec_name, (), sd)
        try:
            assert ("codec_ffn" in eng._demoted) == demoted, (factor, eng._demoted)
            eng.set_precision("f16")
            for stage, T in ((0, 64), (1, 43)):
                x = _inputs(3, T, SPECS[spec_name].dec_channels(stage), torch.Generator().manual_seed(stage), "plain")
                with torch.no_grad():
                    h = CS.rms(x, torch.from_numpy(sd[f"codec.decoder.stages.{stage}.0.ffn_norm.weight"]).double(), 1e-5) @ \
                        torch.from_numpy(sd[f"codec.decoder.stages.{stage}.0.ffn.w1.weight"]).double().t()
                if not demoted:
                    assert float(h.abs().max()) > 200.0   # the pre-activations really are far from the origin
                case = f"w1_x{factor:g}_s{stage}"
                got, _ = _run_hook(eng, D, stage, 4, x)
                assert torch.isfinite(got).all()
                with torch.no_grad():
                    ref = CS.stage(_Lazy64(sd), D, stage, 4, x.float().double(), SPECS[spec_name])
                _assert_within(case, _per_utt(got, ref, x.float().double()), BOUND[("blk", prec_bound)])
        finally:
            eng.close()


def _hook_pipeline(eng, part, x, spec):
    S = spec.n_stages
    for i in range(S):
        x = eng.test_codec_stage(part, i, (1 if i == 0 else 2) | 4 | (8 if i == S - 1 else 0), x)
    return x


@pytest.mark.parametrize("tuning", ["latency", "throughput"])
def test_hook_pipeline_is_the_product_bit_for_bit(tuning):
    """stem -> every stage -> head through the hook equals codec_decode / codec_encode bit for bit at the default precision: the
    hook runs the product's code on the product's plan."""
    from smalltts_amd.engine import DEFAULT_PRECISION
    spec = SPECS["wide"]
    eng = _engine("wide")
    eng.set_precision(DEFAULT_PRECISION)
    eng.set_tuning(tuning)
    try:
        g = torch.Generator().manual_seed(1)
        for B, T in ((2, 3), (8, 75)):
            lat = torch.randn(B, T, 64, generator=g)
            want = eng.codec_decode(lat)
            got = _hook_pipeline(eng, D, lat, spec)
            assert torch.equal(got[..., 0], want[:, 0]), (tuning, B, T)
            audio = torch.randn(B, 1, spec.hop * T, generator=g) * 0.3
            want = eng.codec_encode(audio)
            got = _hook_pipeline(eng, E, audio[:, 0], spec)
            assert torch.equal(got, want), (tuning, B, T)
    finally:
        eng.set_tuning("latency")


BATCH_CASES = [("wide", D, 0, 4, 41), ("wide", D, 3, 2, 7), ("wide", D, 4, 4, 43), ("wide", D, 5, 2, 33), ("wide", D, 6, 4, 33),
               ("wide", D, 6, 8, 85), ("wide", E, 6, 8, 7), ("wide", E, 4, 2, 35), ("c32", D, 1, 4, 64)]


def test_each_utterance_of_a_batch_is_computed_as_alone():
    """A stage on B utterances equals each utterance run alone, bit for bit (no leak across utterance boundaries; these shapes take the
    same kernels at B = 1 and B = 3)."""
    for spec_name, part, stage, what, T in BATCH_CASES:
        spec = SPECS[spec_name]
        eng = _engine(spec_name)
        eng.set_precision("f16")
        x = _inputs(3, T, _in_dims(spec, part, stage, what), torch.Generator().manual_seed(stage), "spikes").float()
        whole = eng.test_codec_stage(part, stage, what, x).cpu()
        for b in range(3):
            alone = eng.test_codec_stage(part, stage, what, x[b: b + 1]).cpu()
            assert torch.equal(alone[0], whole[b]), (spec_name, part, stage, what, b)


def test_hook_refuses_bad_arguments():
    import ctypes as C
    eng = _engine("tiny")
    x = torch.zeros(1, 4, 64, device=eng.device)
    out = torch.empty(1, 64, 64, device=eng.device)
    t, c = C.c_int(0), C.c_int(0)

    def call(part, stage, what, B, T, Cin):
        return eng.lib.smtts_test_codec_stage(eng.h, None, part, stage, what, C.c_void_p(x.data_ptr()), B, T, Cin,
                                              C.c_void_p(out.data_ptr()), C.byref(t), C.byref(c))
    assert call(1, 0, 1, 1, 4, 64) == 0
    for bad in ((3, 0, 1, 1, 4, 64), (1, 9, 4, 1, 4, 64), (1, 0, 2, 1, 4, 64), (1, 1, 1, 1, 4, 64), (1, 0, 1 | 8, 1, 4, 64),
                (1, 1, 2 | 8, 1, 4, 64), (1, 0, 4, 1, 4, 63), (1, 0, 1, 0, 4, 64), (1, 0, 1, 1, 0, 64), (2, 1, 2, 1, 3, 8),
                (1, 0, 16, 1, 4, 64)):
        assert call(*bad) != 0, bad
        assert eng.lib.smtts_last_error(eng.h).decode().startswith("test_codec_stage"), bad


REQUIRED = {
    "codec_chain_wave<32>", "codec_block_wave<32>", "codec_block_wave<64>", "mixer_fused", "mixer_wide", "rmsnorm",
    "dwconv_resid_rms", "dwconv_resid", "codec_ffn_wave<32>", "codec_ffn_wave<64>", "codec_ffn_stream<128>", "codec_ffn_stream<256>",
    "codec_upsample_wave<128x64>", "codec_upsample_wave<256x128>", "to_split", "splitk_resid", "stem_conv1", "head_conv",
    "codec_chain_wave<32> nb=2", "codec_chain_wave<32> nb=3",   # (labels test_stage_vs_fp64 adds: the profiler name has no nb)
}
REQUIRED_PREFIX = {
    "gemm3<160x128,": "160x128 split-K second FFN product",
    "gemm3<64x64,": "64x64 split-K (FFN at M <= 480, encoder strided conv / head)",
    "gemm<": "fp32-A kernel (stem, ConvTranspose, strided conv, head, hidden)",
}


def test_every_kernel_class_was_held_to_fp64():
    """The kernel classes the cases above launched include every codec path.  A dispatch change that leaves a kernel untested fails
    here instead of passing silently.

    It reads what the tests above recorded in this module (SEEN, MEASURED), so it must run after them, as it does in file order, and
    only means something when all of them ran: under a selection (-k, a single test) that left any of them out it skips.  The
    profiler names the streaming and the LDS-staged mixer_fused alike; the two child-process runs of
    test_mixer_segment_lengths_and_staged_mixer_vs_fp64 cover one each by construction."""
    ran = set(MEASURED)
    wanted = set(CASES) | {f"mixer_stream_{m}_s{s}" for m in ("122", "0") for s in (3, 4)} | \
        {f"w1_x{f}_s{s}" for f in ("300", "30000") for s in (0, 1)}
    if not wanted <= ran:
        pytest.skip(f"{len(wanted - ran)} of the cases this check needs did not run in this session")
    print("\n[codec kernels] worst rel err per case (bound):")
    for k, (e, b) in sorted(MEASURED.items()):
        print(f"  {k:40s} {e:.3e}  ({b:.1e})")
    print("[codec kernels] classes seen:", sorted(SEEN))
    missing = sorted(REQUIRED - SEEN)
    assert not missing, missing
    for p, what in REQUIRED_PREFIX.items():
        assert any(n.startswith(p) for n in SEEN), what
    assert any(n.startswith("gemm3<") and ",s4," in n for n in SEEN), "f16x2 ConvTranspose"
    assert any(n.startswith("gemm<") and "gelu" in n for n in SEEN), "fp32-A hidden (F % 64 != 0 / C = 32 unfused)"
