"""ctypes loader for libsmalltts_hip.so (the C ABI declared in include/smalltts_hip.h).

The product path has no CPU fallback: if the shared library is missing or cannot be
loaded, importing an operator raises immediately."""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SMTTS_LIB") or os.path.join(_HERE, "libsmalltts_hip.so")  # SMTTS_LIB: A/B builds (csrc/Makefile)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "smalltts_hip.h")

_lib = None
ABI_VERSION = 11  # include/smalltts_hip.h SMTTS_ABI_VERSION

vp, i32, i64, u64, f32, sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_size_t
u32 = C.c_uint32
cstr = C.c_char_p

# the codes of include/smalltts_hip.h that the host side passes by name (engine.py, engine_hooks.py)
ACT = {"none": 0, "silu": 1, "gelu": 2, "mish": 3}
PRECISION = {"bf16x3": 3, "f16": 2, "bf16": 1,   # presets of smtts_set_precision
             "f16x2": 4}                          # site value only (codec_conv): fp16 activations x fp16 hi + lo weights, two MFMA passes
PRESETS = ("bf16x3", "f16", "bf16")              # what set_precision accepts in front of the site overrides
SITES = {"dit_block": 0, "encoder": 1, "cross_kv": 2, "cond": 3, "codec_ffn": 4, "codec_conv": 5, "convpos": 6, "attn": 7}


def ptr(t):
    """A tensor (or None) as the void * the C ABI takes."""
    return None if t is None else C.c_void_p(t.data_ptr())

# name -> (restype, argtypes); kept in sync with include/smalltts_hip.h (tests/test_cabi.py checks it)
SIGNATURES: Dict[str, Tuple[object, List[object]]] = {
    "smtts_create": (i32, [i32, C.POINTER(vp)]),
    "smtts_destroy": (i32, [vp]),
    "smtts_last_error": (cstr, [vp]),
    "smtts_version": (cstr, []),
    "smtts_abi_version": (i32, []),
    "smtts_get_saturations": (i32, [vp, C.POINTER(C.c_uint32), i32, i32]),
    "smtts_peek_saturations": (i32, [vp, C.POINTER(C.c_uint32), i32]),
    "smtts_range_report": (cstr, [vp]),
    "smtts_range_worst_bound": (f32, [vp]),
    "smtts_set_tensor": (i32, [vp, cstr, vp, C.POINTER(i64), i32, i32]),
    "smtts_synth_tensor": (i32, [vp, cstr, C.POINTER(i64), i32, u64, f32, f32]),
    "smtts_get_tensor": (i32, [vp, cstr, vp, i64]),
    "smtts_set_codec_spec": (i32, [vp, i32, i32, i32, i32, f32, C.POINTER(i32), i32, C.POINTER(i32)]),
    "smtts_finalize": (i32, [vp]),
    "smtts_set_precision": (i32, [vp, i32]),
    "smtts_get_precision": (i32, [vp]),
    "smtts_default_precision": (i32, []),
    "smtts_set_site_precision": (i32, [vp, i32, i32]),
    "smtts_has_part": (i32, [vp, i32]),
    "smtts_cond_workspace_bytes": (sz, [vp, i32, i32, i32]),
    "smtts_cond_encode": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
    "smtts_denoise_workspace_bytes": (sz, [vp, i32, i32, i32, i32]),
    "smtts_denoise_step": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, sz]),
    "smtts_sample_workspace_bytes": (sz, [vp, i32, i32, i32, i32, i32, i32]),
    "smtts_sample": (i32, [vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, u64,
                           vp, vp, vp, sz]),
    "smtts_sample_align": (i32, [vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, u64,
                                 vp, vp, vp, sz, vp, u32, u32, vp]),
    "smtts_sample_pinned": (i32, [vp, vp, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, u64,
                                  vp, vp, vp, sz, vp, u32, u32, vp, vp, vp, i32]),
    "smtts_asr_workspace_bytes": (sz, [vp, i32, i32]),
    "smtts_asr_logprobs": (i32, [vp, vp, vp, vp, i32, i32, vp, sz, vp]),
    "smtts_ctc_score": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "smtts_ctc_greedy": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp]),
    "smtts_ctc_align": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "smtts_ctc_align_long_workspace_bytes": (sz, [vp, i32, i32, i32]),
    "smtts_ctc_align_long": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, sz]),
    "smtts_sv_workspace_bytes": (sz, [vp, i32, i32]),
    "smtts_sv_embed": (i32, [vp, vp, vp, vp, i32, i32, vp, sz, vp]),
    "smtts_sv_cosine": (i32, [vp, vp, vp, vp, i32, i32, i32, vp]),
    "smtts_align_path": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "smtts_take_scores": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, f32, f32, f32, vp, vp]),
    "smtts_take_select": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "smtts_repair_plan": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, i32, i32, vp, vp]),
    "smtts_repair_keep": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "smtts_codec_hop": (i32, [vp]),
    "smtts_decode_workspace_bytes": (sz, [vp, i32, i32]),
    "smtts_codec_decode": (i32, [vp, vp, vp, i32, i32, vp, vp, sz]),
    "smtts_decode_state_bytes": (sz, [vp]),
    "smtts_decode_stream_workspace_bytes": (sz, [vp, i32, i32]),
    "smtts_codec_decode_stream": (i32, [vp, vp, vp, i32, i32, vp, i64, vp, vp, vp, sz]),
    "smtts_test_carry_frames": (i32, [vp, vp, vp, i32, i32, i32, vp, i64, i64, vp]),
    "smtts_encode_workspace_bytes": (sz, [vp, i32, i32]),
    "smtts_codec_encode": (i32, [vp, vp, vp, i32, i32, vp, vp, sz]),
    "smtts_set_dual_stream": (i32, [vp, i32]),
    "smtts_set_tuning": (i32, [vp, i32]),
    "smtts_randn": (i32, [vp, vp, vp, i64, u64, u64]),
    "smtts_resample_poly": (i32, [vp, vp, vp, i32, i64, vp, i32, i32, i32, i32, vp, i64]),
    "smtts_pcm16": (i32, [vp, vp, vp, i64, vp]),
    "smtts_deliver_state_bytes": (sz, [vp, i32]),
    "smtts_deliver": (i32, [vp, vp, vp, i32, i64, vp, vp, i32, i32, i32, i32, vp, i64, i32, vp, i64]),
    "smtts_watermark_state_bytes": (sz, [vp]),
    "smtts_watermark": (i32, [vp, vp, vp, i32, i64, vp, u64, f32, vp, i64, vp]),
    "smtts_watermark_detect_workspace_bytes": (sz, [vp, i32, i64]),
    "smtts_watermark_detect": (i32, [vp, vp, vp, i32, i64, vp, u64, i64, i32, vp, sz, vp, vp, vp, vp, vp]),
    "smtts_voice_expand": (i32, [vp, vp, vp, i32, i32, vp, vp, vp]),
    "smtts_randn_rows": (i32, [vp, vp, vp, vp, vp, i32, i32, i32]),
    "smtts_stitch": (i32, [vp, vp, vp, i32, i64, vp, vp, vp, i32, vp, i64, i32]),
    "smtts_endpoints": (i32, [vp, vp, vp, i32, i64, vp, i32, f32, f32, i32, i32, i32, f32, f32, f32, vp, vp, vp, vp]),
    "smtts_stitch_seg": (i32, [vp, vp, vp, i32, i64, vp, vp, vp, vp, i32, vp, i64, i32]),
    "smtts_join_stream": (i32, [vp, vp, vp, i32, i64, vp, vp, vp, i32, i64, i32, vp, vp, i64, i32, vp, vp, vp, i64]),
    "smtts_retime": (i32, [vp, vp, vp, i32, i64, vp, vp, vp, i32, vp, i32, i32, vp, i64, vp]),
    "smtts_pitch_workspace_bytes": (sz, [vp, i32, i64, i32, i32, i32]),
    "smtts_pitch": (i32, [vp, vp, vp, i32, i64, vp, vp, i32, i32, i32, i32, f32, f32, f32, f32, vp, vp, vp, vp, sz]),
    "smtts_alpha_sigma": (None, [f32, C.POINTER(f32), C.POINTER(f32)]),
    "smtts_profile_enable": (i32, [vp, i32]),
    "smtts_profile_report": (i32, [vp, C.c_char_p, sz]),
    "smtts_bench_gemm": (i32, [vp, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(f32)]),
    "smtts_test_gemm3": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    "smtts_test_ln_fold": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, i32, i32, i32,
                                 vp, vp, vp]),
    "smtts_test_codec_stage": (i32, [vp, vp, i32, i32, i32, vp, i32, i32, i32, vp, C.POINTER(i32), C.POINTER(i32)]),
    "smtts_test_dit_stage": (i32, [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, i32, i32, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp,
                                   vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "smtts_test_scorer_tap_bytes": (sz, [vp, i32, i32, i32, C.POINTER(sz), i32]),
    "smtts_test_scorer_taps": (i32, [vp, vp, i32, vp, vp, i32, i32, vp, vp, sz]),
    "smtts_test_set_fused_ffn": (i32, [vp, i32]),
    "smtts_test_set_ln_fold": (i32, [vp, i32]),
    "smtts_test_gemm": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, vp, i32]),
    "smtts_test_swiglu": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "smtts_test_set_attention_mfma": (i32, [vp, i32]),
    "smtts_test_attention_mfma": (i32, [vp, vp, vp, vp, vp, f32, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, i32,
                                        i32, i32, vp]),
    "smtts_test_attn_text_mass": (i32, [vp, vp, vp, vp, vp, f32, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, i32,
                                        i32, i32, vp]),
    "smtts_test_attention": (i32, [vp, vp, vp, vp, vp, f32, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, i32, i32,
                                   i32, i32, vp]),
}


def header_symbols() -> List[str]:
    """Entry points declared in include/smalltts_hip.h."""
    with open(HEADER_PATH) as f:
        txt = f.read()
    return sorted(set(re.findall(r"\b(smtts_[a-z_0-9]+)\s*\(", txt)))


def load():
    """Load the HIP library; raises if it was not built (python __graft_entry__.py / make -C smalltts_amd/csrc)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `make -C smalltts_amd/csrc` or `python -c 'import __graft_entry__ as g; g.build()'`.")
    # PyTorch-ROCm first: it brings its own copy of the HIP runtime (torch/lib/libamdhip64.so), and this library must bind to THAT one —
    # two HIP runtimes in one process do not both see the GPU.  Loaded the other way round (this library, then torch: what
    # `python __graft_entry__.py smoke` does when build() runs in front of smoke()) smtts_create fails with "no ROCm-capable device".
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.smtts_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has ABI version {lib.smtts_abi_version()}, this host side was written for {ABI_VERSION} "
                           "(include/smalltts_hip.h SMTTS_ABI_VERSION): rebuild with `make -C smalltts_amd/csrc`")
    _lib = lib
    return lib
