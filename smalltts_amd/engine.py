"""Python face of the gfx950 engine: torch-ROCm tensors in, raw HIP underneath.

PyTorch is used only as the device allocator / stream owner; every operator goes through the
C ABI of libsmalltts_hip.so (include/smalltts_hip.h).  One HipEngine per GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, Optional

import numpy as np
import torch

from . import _lib
from ._lib import ACT, PRECISION, PRESETS, SITES, ptr as _p   # noqa: F401  (the codes stay importable from here)
from .engine_hooks import EngineHooks
from .options import as_pitch
from .plans import long_windows, pitch_tables, retime_window
from .operands import (ALIGN_MAX_FRAMES, ALIGN_MAX_TOKENS, distinct_slots, fade_len, frames_tokens, is_operand, out_1d, per_row,
                       pool_slots, row_lengths, seg_gain, upload)
from .weights import (DEFAULT_CODEC, CodecSpec, asr_param_specs, codec_decoder_param_specs, codec_encoder_param_specs,
                      dit_param_specs, init_rule, sv_param_specs, tensor_key)

N_LAYERS, N_HEADS, HEAD_DIM, LATENT = 12, 8, 120, 64
DEFAULT_PRECISION = "f16"
ASR_MAX_ROWS, ASR_UPSAMPLE, ASR_CLASSES = 64, 4, 198   # smtts_asr_logprobs: rows per call, frames per latent frame, phoneme classes
CTC_ALIGN_MAX_FRAMES = 1024                            # smtts_ctc_align: frames of logp per row (its move table lives in LDS)
CTC_LONG_MAX_ROWS, CTC_LONG_MAX_FRAMES, CTC_LONG_MAX_TOKENS = 64, 65536, 16383   # smtts_ctc_align_long (moves in the workspace)
ASR_LONG_MAX_FRAMES = CTC_LONG_MAX_FRAMES // ASR_UPSAMPLE                       # asr_logprobs_long: latent frames of one recording
SV_MAX_ROWS, SV_MIN_FRAMES, SV_DIM = 64, 6, 192       # smtts_sv_embed: rows per call, the shortest row with an embedding, its width


def _index_mask(sel, n: int, what: str) -> int:
    """None -> all n bits; else the bit mask of the indices in `sel` (each in [0, n))."""
    if sel is None:
        return (1 << n) - 1
    idx = [int(i) for i in sel]
    if not idx or any(i < 0 or i >= n for i in idx):
        raise ValueError(f"alignment: {what} must be a non-empty selection of indices in [0, {n}), got {list(sel)}")
    m = 0
    for i in idx:
        m |= 1 << i
    return m


def tap_selection(align, num_steps: int):
    """The tap selection of smtts_sample_align from an `align=` value: True = every layer and head at the last step; else an object
    with .layers / .heads / .steps (None = the default of each; steps index range(num_steps), negative from the end).
    -> (ctypes uint8[num_steps] step flags, layer bit mask, head bit mask).  Host only."""
    layers = None if align is True else getattr(align, "layers", None)
    heads = None if align is True else getattr(align, "heads", None)
    steps = None if align is True else getattr(align, "steps", None)
    if align is not True and not all(hasattr(align, k) for k in ("layers", "heads", "steps")):
        raise TypeError(f"align must be None, a bool or an object with layers / heads / steps, got {type(align).__name__}")
    num_steps = int(num_steps)
    flags = (C.c_uint8 * num_steps)()
    if steps is None:
        flags[num_steps - 1] = 1
    else:
        idx = [int(i) for i in steps]
        if not idx or any(i < -num_steps or i >= num_steps for i in idx):
            raise ValueError(f"alignment: steps must be a non-empty selection of indices in [-{num_steps}, {num_steps}), got {list(steps)}")
        for i in idx:
            flags[i % num_steps] = 1
    return flags, _index_mask(layers, N_LAYERS, "layers"), _index_mask(heads, N_HEADS, "heads")


class HipEngine(EngineHooks):
    def __init__(self, device: int = 0, precision: str = DEFAULT_PRECISION):
        if not torch.cuda.is_available():
            raise RuntimeError("HipEngine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = _lib.load()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        h = C.c_void_p()
        if self.lib.smtts_create(self.device_index, C.byref(h)) != 0:
            raise RuntimeError("smtts_create: " + self.lib.smtts_last_error(None).decode())
        self.h = h
        self._ws: Optional[torch.Tensor] = None
        self._ws_named: Dict[str, torch.Tensor] = {}
        self._ws_slot: Optional[str] = None   # set via use_workspace(): separate scratch per concurrent stream
        self.codec_spec: CodecSpec = DEFAULT_CODEC
        self._banks: Dict[tuple, tuple] = {}   # (down, up) -> (polyphase bank on the device, width)
        self._retime_wins: Dict[int, torch.Tensor] = {}   # hop -> the cross-fade window on the device (plans.retime_window)
        self._pitch_tabs: Dict[tuple, torch.Tensor] = {}  # (lmin, lmax, tilt) -> lg / tilt on the device (plans.pitch_tables)
        self._demoted: Dict[str, str] = {}     # site -> why: sites the fp16 range guard moved to split-bf16 (sticky across set_precision)
        self.calibration: Optional[Dict[str, object]] = None   # last calibrate() report on the loaded weights
        self.dual_stream = os.environ.get("SMTTS_SINGLE_STREAM", "") != "1"   # what the library starts with (set_dual_stream)
        self.tuning, self.ln_fold, self._profiling = "latency", True, False
        self.set_precision(precision)

    # ---- plumbing ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.lib.smtts_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what}: {self.lib.smtts_last_error(self.h).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def use_workspace(self, slot: Optional[str]):
        """Select a named scratch buffer for subsequent calls (ops running concurrently on different streams must
        not share scratch). None = the default buffer."""
        if slot is not None and self._profiling:
            raise RuntimeError("per-kernel profiling is on: it pairs HIP events around every launch and assumes ONE call at a "
                               "time — no batches in flight (include/smalltts_hip.h, threading rule 3)")
        self._ws_slot = slot

    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws_slot is not None:
            w = self._ws_named.get(self._ws_slot)
            if w is None or w.numel() < nbytes:
                self._ws_named[self._ws_slot] = w = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            return w
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._ws

    def _dev(self, t, dtype) -> torch.Tensor:
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _is(self, t, dtype, *shape, aligned: bool = False) -> bool:
        """t is a contiguous `dtype` tensor of `shape` (None: any extent; no shape: any rank) on the engine's device."""
        return is_operand(t, dtype, shape or None, self.device, aligned)

    def _upload_i32(self, rows) -> torch.Tensor:
        """Rows of host integers -> device int32 on the current stream (operands.upload)."""
        return upload([[int(v) for v in r] for r in rows], np.int32, self.device)

    def _upload_i64(self, rows) -> torch.Tensor:
        return upload(rows, np.int64, self.device)

    def set_dual_stream(self, on: bool) -> bool:
        """Text encoder of cond_encode on the engine's side stream (default unless SMTTS_SINGLE_STREAM=1) or inline on the
        caller's stream.  Returns the previous setting so that callers can restore it."""
        prev = self.dual_stream
        self._ck(self.lib.smtts_set_dual_stream(self.h, int(bool(on))), "set_dual_stream")
        self.dual_stream = bool(on)
        return prev

    def set_tuning(self, mode: str) -> str:
        """"latency" (default) or "throughput" (several batches in flight on the caller's streams); returns the previous mode."""
        prev = self.tuning
        self._ck(self.lib.smtts_set_tuning(self.h, {"latency": 0, "throughput": 1}[mode]), "set_tuning")
        self.tuning = mode
        return prev

    def release_workspaces(self):
        """Drop the named per-stream scratch buffers (synthesize_batches / bench keep one per batch in flight)."""
        self._ws_named.clear()

    def set_precision(self, precision: str):
        """Preset ("f16" mixed / "bf16x3" / "bf16"), optionally followed by per-site overrides: "f16,codec_ffn=bf16x3".
        Sites the fp16 range guard demoted (check_fp16_range) stay at split-bf16 whatever the preset says."""
        preset, *over = precision.split(",")
        if preset not in PRESETS:
            raise ValueError(f"precision preset {preset!r}: one of {PRESETS} (\"f16x2\" is a value of the codec_conv site only)")
        self.precision = precision
        self._ck(self.lib.smtts_set_precision(self.h, PRECISION[preset]), "set_precision")
        for o in over:
            site, prec = o.split("=")
            self._ck(self.lib.smtts_set_site_precision(self.h, SITES[site.strip()], PRECISION[prec.strip()]), "set_site_precision")
        for site in self._demoted:
            self._ck(self.lib.smtts_set_site_precision(self.h, SITES[site], PRECISION["bf16x3"]), "set_site_precision")

    # ---- fp16 range guard (include/smalltts_hip.h smtts_get_saturations) ----------------------------------------------
    def saturations(self, reset: bool = True) -> Dict[str, int]:
        """site -> number of values an fp16 producer clamped to +-65504 since the last reset (+ for codec_ffn the fused FFN
        blocks whose range could not be certified from the weights).  Synchronises the device."""
        n = len(SITES)
        buf = (C.c_uint32 * n)()
        self._ck(self.lib.smtts_get_saturations(self.h, buf, n, int(bool(reset))), "get_saturations")
        return {name: int(buf[i]) for name, i in SITES.items()}

    def saturations_now(self) -> Dict[str, int]:
        """saturations() as the counters stand, next to batches in flight on other streams: no device-wide wait and no reset
        (smtts_peek_saturations).  Work that had completed before the call is counted in full."""
        n = len(SITES)
        buf = (C.c_uint32 * n)()
        self._ck(self.lib.smtts_peek_saturations(self.h, buf, n), "peek_saturations")
        return {name: int(buf[i]) for name, i in SITES.items()}

    def check_fp16_range(self, what: str = "", *, in_flight: bool = False) -> list:
        """Reads the saturation counters; every site that clamped is switched to split-bf16 (fp32 range) for the rest of this
        engine's life and a RuntimeWarning says so.  Returns the sites demoted by THIS call: the caller should run the
        operation again — its results were clipped.  in_flight=True reads with saturations_now(): the caller has waited for the work
        it verifies and keeps other batches running (a clamp of theirs, seen early, demotes as well)."""
        import warnings
        counts = self.saturations_now() if in_flight else self.saturations(reset=True)
        hit = {k: v for k, v in counts.items() if v and k not in self._demoted}
        for site, count in hit.items():
            rep = self.lib.smtts_range_report(self.h).decode() if site == "codec_ffn" else ""
            self._demoted[site] = f"{count} clamp(s)" + (f"; {rep}" if rep else "")
            self._ck(self.lib.smtts_set_site_precision(self.h, SITES[site], PRECISION["bf16x3"]), "set_site_precision")
            warnings.warn(f"fp16 range guard{' (' + what + ')' if what else ''}: site {site!r} clamped {count} value(s) to +-65504"
                          f"{' [' + rep.strip('; ') + ']' if rep else ''}; the site now runs split-bf16 (fp32 range, ~3x its MFMA passes)",
                          RuntimeWarning, stacklevel=3)
        return list(hit)

    def calibrate(self, tol: float = 4e-4, codec_snr_db: float = 62.0, seed: int = 1234) -> Dict[str, object]:
        """Checks the precision preset in force ON THE WEIGHTS THAT ARE LOADED: one seeded probe batch (B = 2, N = 40, R = 10,
        P = 12, four DMD steps; six frames through the decoder) at the preset against the same batch at split-bf16 (fp32-class
        operands).  The synthetic recipe's tensors are outlier-free; real checkpoints are not, and "massive" hidden units make
        every 11-bit operand rounding that follows them count for more (tools/outlier_ladder.py: rows of ff.w1 / ff.w3 x30 take
        the fp16 DiT blocks from 1.3e-4 to 2e-2 WITHOUT a single clamp, so the saturation counters alone do not see it).  While
        the latents differ by more than `tol` (rel-L2; the contract vs fp32 is 1e-3) the sites are moved to split-bf16 in the
        order of their measured impact (dit_block, attn, encoder, cross_kv, then everything); likewise codec_ffn / codec_conv
        against `codec_snr_db`.  Demotions are sticky (set_precision keeps them).  Returns what was measured and done."""
        import warnings

        def rel(a, b):
            return float((a - b).double().norm() / b.double().norm().clamp_min(1e-30))

        rep: Dict[str, object] = {"tol": tol, "demoted": []}
        keep = self.precision
        g = torch.Generator().manual_seed(seed)
        if self.has("dit"):
            B, N, R, P = 2, 40, 10, 12
            ref = torch.randn(B, R, 64, generator=g)
            ids = torch.randint(1, 198, (B, P), generator=g)
            pm, mask = torch.ones(B, P, dtype=torch.bool), torch.ones(B, N, dtype=torch.bool)
            noise = torch.randn(4, B, N, 64, generator=g)
            rl = torch.full((B,), R)

            def latents():
                return self.sample(self.cond_encode(ref, rl, ids, pm), mask, num_steps=4, noise=noise).clone()

            saved = dict(self._demoted)
            try:
                self._demoted = {}
                self.set_precision("bf16x3")
                want = latents()
            finally:
                self._demoted = saved
                self.set_precision(keep)
            err = rel(latents(), want)
            rep["latent_rel_l2"] = [("as configured", err)]
            hit = self.check_fp16_range("calibrate")
            if hit:   # a site clamped and now runs split-bf16: the ladder below must start from what THAT configuration measures
                err = rel(latents(), want)
                rep["latent_rel_l2"].append((f"after the range guard moved {'+'.join(hit)}", err))
                rep["demoted"] += hit
            for site in ("dit_block", "attn", "encoder", "cross_kv", "cond", "convpos"):
                if err <= tol:
                    break
                if site in self._demoted:
                    continue
                self._demoted[site] = f"calibration: latents {err:.2e} from split-bf16 (> {tol:.0e})"
                self.set_precision(keep)
                err = rel(latents(), want)
                rep["latent_rel_l2"].append((f"+ {site}=bf16x3", err))
                rep["demoted"].append(site)
        if self.has("decoder"):
            lat = torch.randn(1, 6, 64, generator=g)

            def snr():
                got = self.codec_decode(lat).double()
                return float(10 * torch.log10((wav ** 2).sum() / ((got - wav) ** 2).sum().clamp_min(1e-300)))

            saved = dict(self._demoted)
            try:
                self._demoted = {}
                self.set_precision("bf16x3")
                wav = self.codec_decode(lat).double().clone()
            finally:
                self._demoted = saved
                self.set_precision(keep)
            s = snr()
            rep["codec_snr_db"] = [("as configured", s)]
            hit = self.check_fp16_range("calibrate")
            if hit:
                s = snr()
                rep["codec_snr_db"].append((f"after the range guard moved {'+'.join(hit)}", s))
                rep["demoted"] += hit
            for site in ("codec_ffn", "codec_conv"):
                if s >= codec_snr_db:
                    break
                if site in self._demoted:
                    continue
                self._demoted[site] = f"calibration: decode {s:.1f} dB from split-bf16 (< {codec_snr_db:.0f})"
                self.set_precision(keep)
                s = snr()
                rep["codec_snr_db"].append((f"+ {site}=bf16x3", s))
                rep["demoted"].append(site)
        if rep["demoted"]:
            warnings.warn(f"precision calibration: {', '.join(rep['demoted'])} moved to split-bf16 on these weights "
                          f"({rep.get('latent_rel_l2')}, {rep.get('codec_snr_db')})", RuntimeWarning, stacklevel=2)
        rep["precision_in_force"] = self.precision_in_force()
        self.calibration = rep          # kept for /stats and bench.py: published numbers state the precision actually in force
        return rep

    def precision_in_force(self) -> Dict[str, object]:
        """The preset plus every site the range guard / calibration moved to split-bf16 on the loaded weights (and why)."""
        return {"preset": self.precision, "demoted": dict(self._demoted)}

    # ---- weights -------------------------------------------------------------------------------
    def set_codec_spec(self, spec: CodecSpec):
        self.codec_spec = spec
        r = (C.c_int * len(spec.ratios))(*spec.ratios)
        d = (C.c_int * len(spec.dec_depths))(*spec.dec_depths)
        self._ck(self.lib.smtts_set_codec_spec(self.h, spec.latent_dim, spec.n_filters, spec.kernel, spec.ffn_mult,
                                               spec.eps, r, len(spec.ratios), d), "set_codec_spec")

    def set_tensor(self, name: str, arr):
        if isinstance(arr, torch.Tensor):
            t = arr.detach().to(torch.float32).contiguous()
            on_dev = t.is_cuda
            ptr, shape = t.data_ptr(), tuple(t.shape)
        else:
            t = np.asarray(arr, dtype=np.float32, order="C")   # (ascontiguousarray would turn a 0-d scalar into shape (1,))
            on_dev, ptr, shape = False, t.ctypes.data, t.shape
        sh = (C.c_int64 * max(1, len(shape)))(*shape)
        self._ck(self.lib.smtts_set_tensor(self.h, name.encode(), C.c_void_p(ptr), sh, len(shape), int(on_dev)),
                 f"set_tensor({name})")

    def load_state_dict(self, sd: Dict[str, object]):
        for k, v in sd.items():
            self.set_tensor(k, v)

    def load_synthetic(self, seed: int, parts: Iterable[str] = ("dit", "decoder", "encoder"),
                       codec_spec: Optional[CodecSpec] = None):
        """Fill weights on the GPU with the seeded recipe of weights.py (bit-identical to numpy)."""
        spec = codec_spec or self.codec_spec
        specs = []
        if "dit" in parts:
            specs += dit_param_specs()
        if "decoder" in parts or "encoder" in parts:
            self.set_codec_spec(spec)
        if "decoder" in parts:
            specs += codec_decoder_param_specs(spec)
        if "encoder" in parts:
            specs += codec_encoder_param_specs(spec)
        if "asr" in parts:
            specs += asr_param_specs()
        if "sv" in parts:
            specs += sv_param_specs()
        for name, shape in specs:
            mean, hr = init_rule(name, shape)
            sh = (C.c_int64 * max(1, len(shape)))(*shape)
            self._ck(self.lib.smtts_synth_tensor(self.h, name.encode(), sh, len(shape),
                                                 C.c_uint64(tensor_key(name, seed)), mean, hr), f"synth({name})")

    def get_tensor(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, dtype=np.float32)
        self._ck(self.lib.smtts_get_tensor(self.h, name.encode(), C.c_void_p(out.ctypes.data), out.size), "get_tensor")
        return out

    def finalize(self):
        # demotions were measured on the PREVIOUS weights (C++ resets its static counters and range report in smtts_finalize too):
        # one bad checkpoint must not pin the engine at split-bf16 for its lifetime
        if self._demoted:
            self._demoted = {}
            self.set_precision(self.precision)
        self.calibration = None
        self._ck(self.lib.smtts_finalize(self.h), "finalize")
        self.check_fp16_range("finalize")   # static part: fused codec FFN blocks whose range the weights do not certify

    def has(self, part: str) -> bool:
        return bool(self.lib.smtts_has_part(self.h, {"dit": 0, "decoder": 1, "encoder": 2, "asr": 3, "sv": 4}[part]))

    # ---- operators -----------------------------------------------------------------------------
    def cond_encode(self, ref, ref_len, ids, ph_mask, debug: bool = False) -> Dict[str, torch.Tensor]:
        """(ref (B,R,64), ref_len (B,), ids (B,P), ph_mask (B,P)) -> cross-KV cache
        (reference operator: condition_encoder.onnx, infer/onnx.py:91-96)."""
        ref = self._dev(ref, torch.float32)
        ref_len = self._dev(ref_len, torch.int64)
        ids = self._dev(ids, torch.int64)
        ph_mask = self._dev(ph_mask, torch.bool)
        B, R, _ = ref.shape
        P = ids.shape[1]
        dev = self.device
        out = {
            "k_ref": torch.empty(N_LAYERS, B, N_HEADS, R, HEAD_DIM, device=dev),
            "v_ref": torch.empty(N_LAYERS, B, N_HEADS, R, HEAD_DIM, device=dev),
            "ref_mask": torch.zeros(B, R, dtype=torch.bool, device=dev),
            "k_text": torch.empty(N_LAYERS, B, N_HEADS, P, HEAD_DIM, device=dev),
            "v_text": torch.empty(N_LAYERS, B, N_HEADS, P, HEAD_DIM, device=dev),
            "ph_mask": ph_mask,
        }
        if debug:
            out["ref_seq"] = torch.empty(B, R, 960, device=dev)
            out["phoneme_mem"] = torch.empty(B, P, 960, device=dev)
        nb = self.lib.smtts_cond_workspace_bytes(self.h, B, R, P)
        ws = self._workspace(nb)
        self._ck(self.lib.smtts_cond_encode(self.h, self._stream(), _p(ref), _p(ref_len), _p(ids), _p(ph_mask), B, R, P,
                                            _p(out["k_ref"]), _p(out["v_ref"]), _p(out["ref_mask"]), _p(out["k_text"]),
                                            _p(out["v_text"]), _p(ws), ws.numel(), _p(out.get("ref_seq")),
                                            _p(out.get("phoneme_mem"))), "cond_encode")
        return out

    def denoise_step(self, x_t, mask, t, cache, rope=None) -> torch.Tensor:
        """velocity = denoiser(x_t, mask, t, cache...) (reference operator: denoiser.onnx, infer/onnx.py:107-124)."""
        x_t = self._dev(x_t, torch.float32)
        mask = self._dev(mask, torch.bool)
        t = self._dev(t, torch.float32)
        rope = None if rope is None else self._dev(rope, torch.float32)
        B, N, _ = x_t.shape
        R, P = cache["k_ref"].shape[3], cache["k_text"].shape[3]
        v = torch.empty_like(x_t)
        ws = self._workspace(self.lib.smtts_denoise_workspace_bytes(self.h, B, N, R, P))
        self._ck(self.lib.smtts_denoise_step(self.h, self._stream(), _p(x_t), _p(mask), _p(t), _p(cache["k_ref"]),
                                             _p(cache["v_ref"]), _p(cache["ref_mask"]), _p(cache["k_text"]),
                                             _p(cache["v_text"]), _p(cache["ph_mask"]), _p(rope), B, N, R, P, _p(v),
                                             _p(ws), ws.numel()), "denoise_step")
        return v

    def sample(self, cache, mask, num_steps: int = 4, mode: str = "dmd", cfg: bool = False, s_text: float = 2.0,
               s_spk: float = 1.5, noise=None, seed: int = 0, return_steps: bool = False, align=None, x_pin=None, pin=None,
               start_step: int = 0):
        """Runs the whole sampler on the GPU. mask: (B,N) (cfg: rows are replicated x3 internally).
        x_pin fp32 (B,N,64), pin bool (B,N), start_step (smtts_sample_pinned; the definition: include/smalltts_hip.h; DMD mode without
        cfg only): the frames with pin && mask come back as x_pin, bit for bit, and stay x_pin after every step, so that the other
        frames are denoised with them in view; start_step = k > 0 starts the loop at step k from x_pin (step i always draws noise
        stream i) and leaves the slots below k of the returned steps at zero.  Returns as without them.  Only the mechanism is
        verified: how well the 4-step student inpaints is unvalidated on trained weights (api.SmallTTS.respeak).
        align (None / False: off; True or an object with .layers / .heads / .steps, e.g. api.Alignment): the text-attention tap of
        smtts_sample_align runs behind the selected (step, layer) attention launches and the call returns (x, mass) — with
        return_steps (x, steps, mass) — mass fp32 (B,N,P) on the device: the mean over the selected (step, layer, head) triples of
        each frame's softmax probability on each text key.  x is bit-identical with and without it."""
        mask = self._dev(mask, torch.bool)
        B, N = mask.shape
        rows = cache["k_ref"].shape[1]
        if cfg:
            assert rows == 3 * B, "cfg sampling needs a 3B-row condition cache"
            mask_in = mask.repeat(3, 1).contiguous()
        else:
            assert rows == B
            mask_in = mask
        R, P = cache["k_ref"].shape[3], cache["k_text"].shape[3]
        noise = None if noise is None else self._dev(noise, torch.float32)
        if noise is not None:
            want = (num_steps, B, N, LATENT) if mode == "dmd" else (B, N, LATENT)
            assert tuple(noise.shape) == want, f"noise shape {tuple(noise.shape)} != {want}"
        pinned = x_pin is not None or pin is not None or int(start_step) != 0
        if pinned:
            start_step = int(start_step)
            if mode != "dmd" or cfg:
                raise ValueError("sample: x_pin / pin / start_step belong to the DMD sampler without cfg")
            if not 0 <= start_step < num_steps:
                raise ValueError(f"sample: start_step must lie in [0, {num_steps}), got {start_step}")
            if x_pin is None:
                raise ValueError("sample: pin= and start_step > 0 need x_pin")
            for name, t, shape, dt in (("x_pin", x_pin, (B, N, LATENT), (torch.float32, np.float32)),
                                       ("pin", pin, (B, N), (torch.bool, np.bool_))):
                if t is None:
                    continue
                if not hasattr(t, "shape") or tuple(t.shape) != shape or t.dtype not in dt:
                    raise ValueError(f"sample: {name} must be a {'fp32' if name == 'x_pin' else 'bool'} array of shape {shape}, got "
                                     f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
            x_pin = self._dev(x_pin, torch.float32)
            pin = None if pin is None else self._dev(pin, torch.bool)
            if x_pin.data_ptr() % 16:
                x_pin = x_pin.clone()
            if noise is not None and noise.data_ptr() % 16:
                noise = noise.clone()
        x = torch.empty(B, N, LATENT, device=self.device)
        steps = None
        if return_steps:   # a late start writes the slots from start_step on only: the others are zeros
            steps = (torch.zeros if pinned and start_step > 0 else torch.empty)(num_steps, B, N, LATENT, device=self.device)
        ws = self._workspace(self.lib.smtts_sample_workspace_bytes(self.h, B, N, R, P, num_steps, int(cfg)))
        tap = align is not None and align is not False
        flags, layers, heads = tap_selection(align, num_steps) if tap else (None, 0, 0)
        if tap and P < 1:
            raise ValueError("sample: align= needs text keys (P >= 1)")
        mass = torch.empty(B, N, P, device=self.device) if tap else None
        # what the three entries share; smtts_sample_align appends the tap, smtts_sample_pinned the tap (or none) and the pins
        head = (self.h, self._stream(), 0 if pinned else {"dmd": 0, "ode": 1}[mode], num_steps, 0 if pinned else int(cfg), s_text, s_spk,
                _p(mask_in), _p(cache["k_ref"]), _p(cache["v_ref"]), _p(cache["ref_mask"]), _p(cache["k_text"]), _p(cache["v_text"]),
                _p(cache["ph_mask"]), B, N, R, P, _p(noise), C.c_uint64(seed), _p(x), _p(steps), _p(ws), ws.numel())
        tap_args = (C.cast(flags, C.c_void_p) if tap else None, layers, heads, _p(mass))
        if pinned:
            self._ck(self.lib.smtts_sample_pinned(*head, *tap_args, _p(x_pin), _p(pin), start_step), "sample_pinned")
        elif tap:
            self._ck(self.lib.smtts_sample_align(*head, *tap_args), "sample_align")
        else:
            self._ck(self.lib.smtts_sample(*head), "sample")
        res = (x,) + ((steps,) if return_steps else ()) + ((mass,) if tap else ())
        return res if len(res) > 1 else x

    def _mass_front(self, what, mass, *spans):
        """align_path / take_scores / repair_plan: mass fp32 (B,N,P) in the kernels' N / P range and, where given, its spans -> B, N, P."""
        if not self._is(mass, torch.float32, None, None, None):
            raise ValueError(f"{what}: mass must be a contiguous fp32 (B,N,P) tensor on the engine's device")
        B, N, P = (int(v) for v in mass.shape)
        frames_tokens(what, N, P)
        if spans and not self._is(spans[0], torch.int32, B, P, 2):
            raise ValueError(f"{what}: spans must be a contiguous int32 ({B},{P},2) tensor on the engine's device")
        return B, N, P

    def align_path(self, mass: torch.Tensor, ns, p0, p1):
        """Monotone alignment of a text-mass buffer on the device (smtts_align_path; the definition: include/smalltts_hip.h).
        mass fp32 (B,N,P) contiguous on the device, N <= 225, P <= 198; ns frames per row, [p0[b], p1[b]) the tokens the audio
        speaks (host integers).  -> (spans int32 (B,P,2) = (first, last) frame per token, (-1,-1) outside the path; score fp32 (B)),
        both on the device.  One launch on the current stream, no synchronisation."""
        B, N, P = self._mass_front("align_path", mass)
        per_row("align_path", B, ns, p0, p1)
        tab = self._upload_i32([ns, p0, p1])
        spans = torch.empty(B, P, 2, dtype=torch.int32, device=self.device)
        score = torch.empty(B, device=self.device)
        self._ck(self.lib.smtts_align_path(self.h, self._stream(), _p(mass), B, N, P, _p(tab[0]), _p(tab[1]), _p(tab[2]), _p(spans),
                                           _p(score)), "align_path")
        return spans, score

    def asr_logprobs(self, x: torch.Tensor, ns, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-frame phoneme log-probabilities of latents (smtts_asr_logprobs; the definition: include/smalltts_hip.h).
        x fp32 (B,N,64) contiguous on the device, B <= 64, N <= 225; ns the frames per row (host integers).  -> logp fp32 (B,4N,198)
        on the device (out: a contiguous fp32 tensor of that shape to write into), 0.0 at and behind frame 4 ns[b]; every row is
        computed as if it were alone.  Needs the recogniser part (load_synthetic(parts=(..., "asr")) or the asr.* tensors).  Launches
        on the current stream, no synchronisation."""
        return self._score_latents("asr_logprobs", "asr", "recogniser", x, ns, out, ASR_MAX_ROWS, 1, f"N <= {ALIGN_MAX_FRAMES}",
                                   lambda B, N: (B, ASR_UPSAMPLE * N, ASR_CLASSES))

    def sv_embed(self, x: torch.Tensor, ns, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Speaker embedding of every row of latents (smtts_sv_embed; the definition: include/smalltts_hip.h).  x fp32
        (B,N,64) contiguous on the device, B <= 64, 6 <= N <= 225; ns the frames per row (host integers).  -> emb fp32 (B,192) on the
        device (out: a contiguous fp32 tensor of that shape to write into), not normalised; every row is computed as if it were alone,
        and a row under 6 frames has no embedding: its row is 0.0.  Needs the verifier part (load_synthetic(parts=(..., "sv")) or the
        sv.* tensors).  Launches on the current stream, no synchronisation."""
        return self._score_latents("sv_embed", "sv", "verifier", x, ns, out, SV_MAX_ROWS, SV_MIN_FRAMES,
                                   f"{SV_MIN_FRAMES} <= N <= {ALIGN_MAX_FRAMES}", lambda B, N: (B, SV_DIM))

    def _score_latents(self, entry, part, part_name, x, ns, out, max_rows, min_frames, n_range, shape_of):
        """asr_logprobs / sv_embed: the operand checks, the result, the frame table and the workspace of smtts_<entry>."""
        if not self._is(x, torch.float32, None, None, LATENT):
            raise ValueError(f"{entry}: x must be a contiguous fp32 (B,N,64) tensor on the engine's device")
        B, N = int(x.shape[0]), int(x.shape[1])
        if not (1 <= B <= max_rows and min_frames <= N <= ALIGN_MAX_FRAMES):
            raise ValueError(f"{entry}: B = {B}, N = {N} outside the supported range B <= {max_rows}, {n_range}")
        per_row(entry, B, ns)
        if not self.has(part):
            raise ValueError(f"{entry}: this engine holds no {part_name} part")
        want = shape_of(B, N)
        if out is None:
            out = torch.empty(want, device=self.device)
        elif not self._is(out, torch.float32, *want):
            raise ValueError(f"{entry}: out must be a contiguous fp32 {want} tensor on the engine's device")
        tab = self._upload_i32([ns])
        ws = self._workspace(getattr(self.lib, f"smtts_{part}_workspace_bytes")(self.h, B, N))
        self._ck(getattr(self.lib, f"smtts_{entry}")(self.h, self._stream(), _p(x), _p(tab[0]), B, N, _p(ws), ws.numel(), _p(out)), entry)
        return out

    def sv_cosine(self, emb: torch.Tensor, ref: torch.Tensor, K: int = 1) -> torch.Tensor:
        """Cosine of row b of emb against row b // K of ref (smtts_sv_cosine): emb fp32 (B,D) and ref fp32 (B/K,D),
        contiguous on the device, 1 <= K <= 16, D <= 1024.  -> cos fp32 (B) on the device, F.cosine_similarity's rule (each norm clamped
        at 1e-8: a zero row gives 0).  Needs no weights.  One launch on the current stream, no synchronisation."""
        for name, t in (("emb", emb), ("ref", ref)):
            if not self._is(t, torch.float32, None, None):
                raise ValueError(f"sv_cosine: {name} must be a contiguous fp32 2-d tensor on the engine's device")
        B, D = int(emb.shape[0]), int(emb.shape[1])
        K = int(K)
        if not (1 <= K <= 16 and B >= 1 and B % K == 0 and 1 <= D <= 1024):
            raise ValueError(f"sv_cosine: B = {B}, K = {K}, D = {D} outside the supported range 1 <= K <= 16, B % K == 0, 1 <= D <= 1024")
        if tuple(ref.shape) != (B // K, D):
            raise ValueError(f"sv_cosine: ref must have shape ({B // K}, {D})")
        cos = torch.empty(B, device=self.device)
        self._ck(self.lib.smtts_sv_cosine(self.h, self._stream(), _p(emb), _p(ref), B, K, D, _p(cos)), "sv_cosine")
        return cos

    def _ctc_front(self, what, logp, ts, tokens, p0, p1, t_max, p_max=ALIGN_MAX_TOKENS, b_max=None):
        """ctc_score / ctc_align / ctc_align_long: the operand checks (t_max: the most frames, b_max: the most rows, None for no
        limit; p_max: the most tokens) -> (B, T, P, C, the uploaded table)."""
        if not self._is(logp, torch.float32, None, None, None):
            raise ValueError(f"{what}: logp must be a contiguous fp32 (B,T,C) tensor on the engine's device")
        B, T, Cn = (int(v) for v in logp.shape)
        if not self._is(tokens, torch.int32, B, None):
            raise ValueError(f"{what}: tokens must be a contiguous int32 ({B},P) tensor on the engine's device")
        P = int(tokens.shape[1])
        if not (1 <= T <= (t_max or T) and 1 <= P <= p_max and 2 <= Cn <= 256):
            raise ValueError(f"{what}: T = {T}, P = {P}, C = {Cn} outside the supported range "
                             f"{f'1 <= T <= {t_max}' if t_max else 'T >= 1'}, P <= {p_max}, 2 <= C <= 256")
        if b_max is not None and B > b_max:
            raise ValueError(f"{what}: B = {B} rows, at most {b_max} per call")
        per_row(what, B, ts, p0, p1)
        return B, T, P, Cn, self._upload_i32([ts, p0, p1])

    def ctc_score(self, logp: torch.Tensor, ts, tokens: torch.Tensor, p0, p1) -> torch.Tensor:
        """CTC negative log-likelihood of every row (smtts_ctc_score; the definition: include/smalltts_hip.h).  logp fp32
        (B,T,C) and tokens int32 (B,P), contiguous on the device, P <= 198, C <= 256; ts the frames per row, [p0[b], p1[b]) the
        target tokens of row b (host integers).  -> nll fp32 (B) on the device: F.ctc_loss(blank=0, reduction='none'), +inf for an
        empty or infeasible row.  Needs no weights.  One launch on the current stream, no synchronisation."""
        B, T, P, Cn, tab = self._ctc_front("ctc_score", logp, ts, tokens, p0, p1, None)
        nll = torch.empty(B, device=self.device)
        self._ck(self.lib.smtts_ctc_score(self.h, self._stream(), _p(logp), _p(tab[0]), _p(tokens), _p(tab[1]), _p(tab[2]), B, T, P, Cn,
                                          _p(nll)), "ctc_score")
        return nll

    def ctc_align(self, logp: torch.Tensor, ts, tokens: torch.Tensor, p0, p1, frames: bool = False):
        """The best CTC path of every row (smtts_ctc_align; the definition: include/smalltts_hip.h).  Arguments as
        ctc_score, T <= 1024.  -> (spans int32 (B,P,2), the (first, last) frame of logp of every token of [p0[b], p1[b]) and (-1, -1)
        for every other token; tok_logp fp32 (B,P), the path's log-probability per token; score fp32 (B), the path's
        log-probability), and with frames=True a fourth element frame_tok int32 (B,T): the token of every label frame, -1 on blank
        frames and behind ts[b].  A row without frames or tokens, an infeasible row and a NaN score are not aligned: every span
        (-1, -1), tok_logp 0, frame_tok -1, score -inf (or the NaN).  All on the device.  Needs no weights.  One launch on the current
        stream, no synchronisation."""
        B, T, P, Cn, tab = self._ctc_front("ctc_align", logp, ts, tokens, p0, p1, CTC_ALIGN_MAX_FRAMES)
        spans = torch.empty(B, P, 2, dtype=torch.int32, device=self.device)
        tok_logp = torch.empty(B, P, device=self.device)
        score = torch.empty(B, device=self.device)
        frame_tok = torch.empty(B, T, dtype=torch.int32, device=self.device) if frames else None
        self._ck(self.lib.smtts_ctc_align(self.h, self._stream(), _p(logp), _p(tab[0]), _p(tokens), _p(tab[1]), _p(tab[2]), B, T, P, Cn,
                                          _p(spans), _p(tok_logp), _p(frame_tok), _p(score)), "ctc_align")
        return (spans, tok_logp, score, frame_tok) if frames else (spans, tok_logp, score)

    def ctc_align_long(self, logp: torch.Tensor, ts, tokens: torch.Tensor, p0, p1, frames: bool = False):
        """ctc_align for rows past its limits (smtts_ctc_align_long; the definition: smtts_ctc_align's): arguments and
        results as ctc_align, B <= 64, T <= 65536, P <= 16383; wherever both accept a call the results are equal bit for bit.  The
        moves of the lattice go to the engine's workspace: 8 T ceil((2 P + 1) / 32) + 2 T bytes per row, 512 MiB at the limits.
        Needs no weights.  One launch on the current stream, no synchronisation."""
        B, T, P, Cn, tab = self._ctc_front("ctc_align_long", logp, ts, tokens, p0, p1, CTC_LONG_MAX_FRAMES, CTC_LONG_MAX_TOKENS,
                                           CTC_LONG_MAX_ROWS)
        spans = torch.empty(B, P, 2, dtype=torch.int32, device=self.device)
        tok_logp = torch.empty(B, P, device=self.device)
        score = torch.empty(B, device=self.device)
        frame_tok = torch.empty(B, T, dtype=torch.int32, device=self.device) if frames else None
        ws = self._workspace(self.lib.smtts_ctc_align_long_workspace_bytes(self.h, B, T, P))
        self._ck(self.lib.smtts_ctc_align_long(self.h, self._stream(), _p(logp), _p(tab[0]), _p(tokens), _p(tab[1]), _p(tab[2]), B, T, P,
                                               Cn, _p(spans), _p(tok_logp), _p(frame_tok), _p(score), _p(ws), ws.numel()),
                 "ctc_align_long")
        return (spans, tok_logp, score, frame_tok) if frames else (spans, tok_logp, score)

    def asr_logprobs_long(self, x: torch.Tensor, max_rows: int = ASR_MAX_ROWS) -> torch.Tensor:
        """Per-frame phoneme log-probabilities of one recording of any length: x fp32 (N,64) contiguous on the device,
        1 <= N <= 16384 -> logp fp32 (4 N, 198) on the device.  N <= 225: the bits of asr_logprobs.  Longer: windows of 225 latent
        frames every 180 (the last one moved back to end at N, so every window is full; plans.long_windows), each computed as if
        alone by smtts_asr_logprobs, max_rows (1 ... 64) windows per call, in order; latent frame n takes its four recogniser frames
        from the window it lies deeper inside (the cuts are the midpoints of the overlaps).  The result does not depend on
        max_rows.  A frame near a cut has seen its 30 s window, not the whole recording.  Needs the recogniser part.  Launches on
        the current stream, no synchronisation."""
        if not self._is(x, torch.float32, None, LATENT):
            raise ValueError("asr_logprobs_long: x must be a contiguous fp32 (N,64) tensor on the engine's device")
        N, max_rows = int(x.shape[0]), int(max_rows)
        if not 1 <= N <= ASR_LONG_MAX_FRAMES:
            raise ValueError(f"asr_logprobs_long: N = {N} outside the supported range 1 <= N <= {ASR_LONG_MAX_FRAMES}")
        if not 1 <= max_rows <= ASR_MAX_ROWS:
            raise ValueError(f"asr_logprobs_long: max_rows = {max_rows} outside [1, {ASR_MAX_ROWS}]")
        starts, cuts, _ = long_windows(N)
        if len(starts) == 1:
            return self.asr_logprobs(x.unsqueeze(0), [N])[0]
        Wn = ALIGN_MAX_FRAMES
        out = torch.empty(ASR_UPSAMPLE * N, ASR_CLASSES, device=self.device)
        for w0 in range(0, len(starts), max_rows):
            w1 = min(w0 + max_rows, len(starts))
            xs = torch.stack([x[a:a + Wn] for a in starts[w0:w1]])
            lp = self.asr_logprobs(xs, [Wn] * (w1 - w0))
            for w in range(w0, w1):
                a, c0, c1 = starts[w], cuts[w], cuts[w + 1]
                out[ASR_UPSAMPLE * c0:ASR_UPSAMPLE * c1] = lp[w - w0, ASR_UPSAMPLE * (c0 - a):ASR_UPSAMPLE * (c1 - a)]
        return out

    def ctc_greedy(self, logp: torch.Tensor, ts):
        """Greedy CTC transcript of every row (smtts_ctc_greedy): per-frame argmax (lowest class on ties), runs collapsed, class 0
        dropped.  logp fp32 (B,T,C) contiguous on the device, T <= 4096; ts the frames per row (host integers).  -> (ids int32 (B,T),
        zeros behind the count; n_ids int32 (B)), on the device.  Needs no weights.  One launch, no synchronisation."""
        if not self._is(logp, torch.float32, None, None, None):
            raise ValueError("ctc_greedy: logp must be a contiguous fp32 (B,T,C) tensor on the engine's device")
        B, T, Cn = (int(v) for v in logp.shape)
        if not (1 <= T <= 4096 and Cn >= 1):
            raise ValueError(f"ctc_greedy: T = {T}, C = {Cn} outside the supported range 1 <= T <= 4096, C >= 1")
        per_row("ctc_greedy", B, ts)
        tab = self._upload_i32([ts])
        ids = torch.empty(B, T, dtype=torch.int32, device=self.device)
        n_ids = torch.empty(B, dtype=torch.int32, device=self.device)
        self._ck(self.lib.smtts_ctc_greedy(self.h, self._stream(), _p(logp), _p(tab[0]), B, T, Cn, _p(ids), _p(n_ids)), "ctc_greedy")
        return ids, n_ids

    def take_scores(self, mass: torch.Tensor, spans: torch.Tensor, path_score: torch.Tensor, ns, p0, p1, takes):
        """The quality score of every row behind align_path (smtts_take_scores; the definition: include/smalltts_hip.h).
        mass fp32 (B,N,P), spans int32 (B,P,2) and path_score fp32 (B) as sample(align=) / align_path return them, contiguous on the
        device; ns, p0, p1 the host integers align_path was given; takes anything with .weights (four floats >= 0), .tau_token and
        .tau_frame (e.g. api.Takes).  -> (feat int32 (B,4) = (cells, skipped, longest, idle), total fp32 (B), lower is better, +inf
        for an empty row), both on the device.  One launch on the current stream, no synchronisation.  What the total is worth on
        trained weights is unvalidated (api.Takes)."""
        B, N, P = self._mass_front("take_scores", mass, spans)
        if not self._is(path_score, torch.float32, B):
            raise ValueError(f"take_scores: path_score must be a contiguous fp32 ({B},) tensor on the engine's device")
        per_row("take_scores", B, ns, p0, p1)
        w = [float(v) for v in takes.weights]
        tt, tf = float(takes.tau_token), float(takes.tau_frame)
        if len(w) != 4 or not all(v >= 0.0 for v in w) or tt != tt or tf != tf:
            raise ValueError("take_scores: four weights >= 0 and thresholds that are not NaN")
        tab = self._upload_i32([ns, p0, p1])
        feat = torch.empty(B, 4, dtype=torch.int32, device=self.device)
        total = torch.empty(B, device=self.device)
        self._ck(self.lib.smtts_take_scores(self.h, self._stream(), _p(mass), _p(spans), _p(path_score), _p(tab[0]), _p(tab[1]), _p(tab[2]),
                                            B, N, P, tt, tf, w[0], w[1], w[2], w[3], _p(feat), _p(total)), "take_scores")
        return feat, total

    def take_select(self, total: torch.Tensor, K: int, x: torch.Tensor, ns, spans: Optional[torch.Tensor] = None,
                    mass: Optional[torch.Tensor] = None):
        """Keeps the best take of every group on the device (smtts_take_select): rows are piece-major, row = g * K + k, B = G * K.
        total fp32 (B) (take_scores), x fp32 (B,N,64), optionally spans int32 (B,P,2) and mass fp32 (B,N,P), all contiguous on the
        device; ns the B frame counts (host integers).  The winner of group g is the lowest k with the smallest total (NaN counts
        as +inf).  -> (x_win (G,N,64), n_win int32 (G), spans_win (G,P,2) or None, mass_win (G,N,P) or None, winner int32 (G)), on the
        device, the winners' rows bit for bit.  One launch on the current stream, no synchronisation."""
        K = int(K)
        if not self._is(total, torch.float32, None):
            raise ValueError("take_select: total must be a contiguous fp32 (B,) tensor on the engine's device")
        B = int(total.shape[0])
        if not 1 <= K <= 16 or B < 1 or B % K:
            raise ValueError(f"take_select: K must be in [1, 16] and divide the {B} rows")
        G = B // K
        if not self._is(x, torch.float32, B, None, LATENT):
            raise ValueError(f"take_select: x must be a contiguous fp32 ({B},N,{LATENT}) tensor on the engine's device")
        N = int(x.shape[1])
        P = int(spans.shape[1]) if spans is not None and spans.dim() == 3 else int(mass.shape[2]) if mass is not None and mass.dim() == 3 else 1
        frames_tokens("take_select", N, P)
        if spans is not None and not self._is(spans, torch.int32, B, P, 2):
            raise ValueError(f"take_select: spans must be a contiguous int32 ({B},{P},2) tensor on the engine's device, or None")
        if mass is not None and not self._is(mass, torch.float32, B, N, P):
            raise ValueError(f"take_select: mass must be a contiguous fp32 ({B},{N},{P}) tensor on the engine's device, or None")
        per_row("take_select", B, ns)
        tab = self._upload_i32([ns])
        dev = self.device
        x_win = torch.empty(G, N, LATENT, device=dev)
        n_win = torch.empty(G, dtype=torch.int32, device=dev)
        spans_win = None if spans is None else torch.empty(G, P, 2, dtype=torch.int32, device=dev)
        mass_win = None if mass is None else torch.empty(G, N, P, device=dev)
        winner = torch.empty(G, dtype=torch.int32, device=dev)
        self._ck(self.lib.smtts_take_select(self.h, self._stream(), _p(total), G, K, N, P, _p(x), _p(tab[0]), _p(spans), _p(mass),
                                            _p(x_win), _p(n_win), _p(spans_win), _p(mass_win), _p(winner)), "take_select")
        return x_win, n_win, spans_win, mass_win, winner

    def repair_plan(self, mass: torch.Tensor, spans: torch.Tensor, ns, p0, p1, repair, keep: Optional[torch.Tensor] = None):
        """The pin mask that re-speaks only the badly aligned tokens of every row (smtts_repair_plan; the definition:
        include/smalltts_hip.h).  mass fp32 (B,N,P) and spans int32 (B,P,2) as sample(align=) / align_path (or take_select)
        return them, contiguous on the device; ns, p0, p1 the host integers align_path was given; repair anything with .tau_token,
        .max_span and .margin (e.g. api.Repair); keep an optional bool / uint8 (B,N) device tensor of frames that stay pinned whatever
        the plan says.  -> (pin bool (B,N), what sample(pin=) takes: True = keep the frame; counts int32 (B,2) = (bad tokens, freed
        frames)), on the device.  One launch on the current stream, no synchronisation.  How well the freed frames are re-spoken is
        unvalidated on trained weights (api.Repair)."""
        B, N, P = self._mass_front("repair_plan", mass, spans)
        if keep is not None and not self._is(keep, (torch.bool, torch.uint8), B, N):
            raise ValueError(f"repair_plan: keep must be a contiguous bool or uint8 ({B},{N}) tensor on the engine's device, or None")
        per_row("repair_plan", B, ns, p0, p1)
        tt, span, margin = float(repair.tau_token), int(repair.max_span), int(repair.margin)
        if tt != tt or not 1 <= span <= ALIGN_MAX_FRAMES or not 0 <= margin <= 32:
            raise ValueError(f"repair_plan: a threshold that is not NaN, max_span in [1, {ALIGN_MAX_FRAMES}] and margin in [0, 32]")
        tab = self._upload_i32([ns, p0, p1])
        pin = torch.empty(B, N, dtype=torch.bool, device=self.device)       # (one byte per frame, written 0 / 1)
        counts = torch.empty(B, 2, dtype=torch.int32, device=self.device)
        self._ck(self.lib.smtts_repair_plan(self.h, self._stream(), _p(mass), _p(spans), _p(tab[0]), _p(tab[1]), _p(tab[2]), _p(keep), B, N, P,
                                            tt, span, margin, _p(pin), _p(counts)), "repair_plan")
        return pin, counts

    def repair_keep(self, total_cur: torch.Tensor, total_new: torch.Tensor, counts: torch.Tensor, feat_cur: torch.Tensor,
                    feat_new: torch.Tensor, x_cur: torch.Tensor, x_new: torch.Tensor, spans_cur: Optional[torch.Tensor] = None,
                    spans_new: Optional[torch.Tensor] = None, mass_cur: Optional[torch.Tensor] = None,
                    mass_new: Optional[torch.Tensor] = None):
        """Keeps the repaired row only where it is strictly better (smtts_repair_keep): where counts[g][1] > 0 and total_new[g] <
        total_cur[g] (NaN counts as +inf), row g of x_new (G,N,64) and, where given, spans_new (G,P,2) and mass_new (G,N,P) replaces
        row g of x_cur, spans_cur, mass_cur IN PLACE, bit for bit; every other row keeps its bits.  total_* fp32 (G), feat_* int32
        (G,4) (take_scores), counts int32 (G,2) (repair_plan), all contiguous on the device.  -> (total_out (G), feat_out (G,4), kept
        int32 (G)), fresh tensors: those of the row that stays, and the decision.  One launch on the current stream, no
        synchronisation."""
        dev, ok = self.device, self._is
        if not isinstance(total_cur, torch.Tensor) or total_cur.dim() != 1 or int(total_cur.shape[0]) < 1:
            raise ValueError("repair_keep: total_cur must be a contiguous fp32 (G,) tensor on the engine's device")
        G = int(total_cur.shape[0])
        if not (ok(total_cur, torch.float32, G) and ok(total_new, torch.float32, G)):
            raise ValueError(f"repair_keep: total_cur and total_new must be contiguous fp32 ({G},) tensors on the engine's device")
        if not (ok(counts, torch.int32, G, 2) and ok(feat_cur, torch.int32, G, 4) and ok(feat_new, torch.int32, G, 4)):
            raise ValueError(f"repair_keep: counts must be int32 ({G},2) and feat_cur / feat_new int32 ({G},4), contiguous on the engine's device")
        if not ok(x_cur, torch.float32, G, None, LATENT) or not ok(x_new, torch.float32, *x_cur.shape):
            raise ValueError(f"repair_keep: x_cur and x_new must be contiguous fp32 ({G},N,{LATENT}) tensors on the engine's device")
        N = int(x_cur.shape[1])
        if (spans_cur is None) != (spans_new is None) or (mass_cur is None) != (mass_new is None):
            raise ValueError("repair_keep: spans_cur / spans_new and mass_cur / mass_new are given or None together")
        P = (int(spans_cur.shape[1]) if spans_cur is not None and spans_cur.dim() == 3
             else int(mass_cur.shape[2]) if mass_cur is not None and mass_cur.dim() == 3 else 1)
        frames_tokens("repair_keep", N, P)
        if spans_cur is not None and not (ok(spans_cur, torch.int32, G, P, 2) and ok(spans_new, torch.int32, G, P, 2)):
            raise ValueError(f"repair_keep: spans_cur and spans_new must be contiguous int32 ({G},{P},2) tensors on the engine's device, or None")
        if mass_cur is not None and not (ok(mass_cur, torch.float32, G, N, P) and ok(mass_new, torch.float32, G, N, P)):
            raise ValueError(f"repair_keep: mass_cur and mass_new must be contiguous fp32 ({G},{N},{P}) tensors on the engine's device, or None")
        total_out = torch.empty(G, device=dev)
        feat_out = torch.empty(G, 4, dtype=torch.int32, device=dev)
        kept = torch.empty(G, dtype=torch.int32, device=dev)
        self._ck(self.lib.smtts_repair_keep(self.h, self._stream(), G, N, P, _p(total_cur), _p(total_new), _p(counts), _p(feat_cur),
                                            _p(feat_new), _p(x_cur), _p(x_new), _p(spans_cur), _p(spans_new), _p(mass_cur), _p(mass_new),
                                            _p(total_out), _p(feat_out), _p(kept)), "repair_keep")
        return total_out, feat_out, kept

    @property
    def hop(self) -> int:
        return int(self.lib.smtts_codec_hop(self.h))

    def codec_decode(self, latents) -> torch.Tensor:
        """(B,T,64) -> (B,1,hop*T) (reference operator: codec/decoder.onnx, codec/onnx.py:42-53)."""
        lat = self._dev(latents, torch.float32)
        B, T, _ = lat.shape
        audio = torch.empty(B, 1, self.hop * T, device=self.device)
        ws = self._workspace(self.lib.smtts_decode_workspace_bytes(self.h, B, T))
        self._ck(self.lib.smtts_codec_decode(self.h, self._stream(), _p(lat), B, T, _p(audio), _p(ws), ws.numel()),
                 "codec_decode")
        return audio

    # ---- streamed decode: chunks of audio with carried causal state (include/smalltts_hip.h) ------------------------
    @property
    def decode_state_bytes(self) -> int:
        """Bytes of one state slot of a streamed decode (a multiple of 256: the slot stride of a pool)."""
        n = int(self.lib.smtts_decode_state_bytes(self.h))
        if n <= 0:
            raise RuntimeError(f"decode_state_bytes: {self.lib.smtts_last_error(self.h).decode()}")
        return n

    def decode_state(self, n_slots: int) -> torch.Tensor:
        """A zeroed state pool of n_slots streams: uint8 (n_slots, state_bytes) on the device.  A zero slot is the start of an
        utterance; the pool is the caller's: state[k].zero_() resets stream k, state[k].clone() / .copy_() snapshot and rewind it
        (on the stream the decodes run on)."""
        n_slots = int(n_slots)
        if n_slots < 1:
            raise ValueError("decode_state: at least one slot")
        return torch.zeros(n_slots, self.decode_state_bytes, dtype=torch.uint8, device=self.device)

    def codec_decode_stream(self, latents, state: torch.Tensor, slots) -> torch.Tensor:
        """The next chunk of B streams: latents (B,T,64), row b continuing the stream whose state is slot slots[b] of `state`
        (decode_state()) -> audio (B,1,hop*T); the state moves on in place.  The concatenated chunks of a stream are the decode of
        its concatenated latents (smtts_codec_decode_stream).  slots: B distinct host integers in [0, n_slots); the table goes up
        pinned and non-blocking.  On the current stream, no synchronisation."""
        lat = self._dev(latents, torch.float32)
        if lat.dim() != 3 or int(lat.shape[2]) != LATENT or int(lat.shape[0]) < 1 or int(lat.shape[1]) < 1:
            raise ValueError(f"codec_decode_stream: latents must be (B,T,{LATENT}) with B, T >= 1, got {tuple(lat.shape)}")
        B, T, _ = (int(v) for v in lat.shape)
        n_slots = pool_slots("codec_decode_stream", self.device, state, self.decode_state_bytes, "state", "decode_state")
        tab = self._upload_i64(distinct_slots("codec_decode_stream", slots, B, n_slots))
        audio = torch.empty(B, 1, self.hop * T, device=self.device)
        ws = self._workspace(self.lib.smtts_decode_stream_workspace_bytes(self.h, B, T))
        self._ck(self.lib.smtts_codec_decode_stream(self.h, self._stream(), _p(lat), B, T, _p(state), n_slots, _p(tab), _p(audio),
                                                    _p(ws), ws.numel()), "codec_decode_stream")
        return audio

    def codec_encode(self, audio) -> torch.Tensor:
        """(B,1,S) -> (B,S//hop,64) (reference operator: codec/encoder.onnx, codec/onnx.py:64-75)."""
        a = self._dev(audio, torch.float32)
        B, _, S = a.shape
        T = S // self.hop
        S_use = T * self.hop
        if S_use != S:
            a = a[:, :, :S_use].contiguous()
        lat = torch.empty(B, T, LATENT, device=self.device)
        if T == 0:
            return lat
        ws = self._workspace(self.lib.smtts_encode_workspace_bytes(self.h, B, S_use))
        self._ck(self.lib.smtts_codec_encode(self.h, self._stream(), _p(a), B, S_use, _p(lat), _p(ws), ws.numel()),
                 "codec_encode")
        return lat

    def randn(self, n: int, seed: int, stream_id: int = 0) -> torch.Tensor:
        out = torch.empty(n, device=self.device)
        self._ck(self.lib.smtts_randn(self.h, self._stream(), _p(out), n, C.c_uint64(seed), C.c_uint64(stream_id)), "randn")
        return out

    # ---- long-form synthesis: one voice, many rows (include/smalltts_hip.h) -----------------------------
    def voice_expand(self, voices) -> Dict[str, torch.Tensor]:
        """B voices (objects with k_ref / v_ref (12,1,8,R_b,120) fp32 on this device, or such pairs) -> the reference half of a
        cross-KV cache: k_ref, v_ref (12,B,8,Rmax,120) and ref_mask (B,Rmax), bit-identical copies with zeros in the padding.
        The voices' tensors are read on the current stream: keep them alive until that work has completed."""
        pairs = [(v.k_ref, v.v_ref) if hasattr(v, "k_ref") else tuple(v) for v in voices]
        B = len(pairs)
        if B == 0:
            raise ValueError("voice_expand: no voices")
        rows = []
        for k, v in pairs:
            R = int(k.shape[3])
            want = (N_LAYERS, 1, N_HEADS, R, HEAD_DIM)
            for t in (k, v):
                if not self._is(t, torch.float32, *want) or R < 1:
                    raise ValueError(f"voice_expand: a voice's k_ref / v_ref must be contiguous fp32 {want} with R >= 1 on {self.device}, "
                                     f"got {tuple(t.shape)} {t.dtype} on {t.device}")
            rows.append((k.data_ptr(), v.data_ptr(), R))
        Rmax = max(r[2] for r in rows)
        dev = self.device
        out = {"k_ref": torch.empty(N_LAYERS, B, N_HEADS, Rmax, HEAD_DIM, device=dev),
               "v_ref": torch.empty(N_LAYERS, B, N_HEADS, Rmax, HEAD_DIM, device=dev),
               "ref_mask": torch.empty(B, Rmax, dtype=torch.bool, device=dev)}
        table = self._upload_i64(rows)
        self._ck(self.lib.smtts_voice_expand(self.h, self._stream(), _p(table), B, Rmax, _p(out["k_ref"]), _p(out["v_ref"]),
                                             _p(out["ref_mask"])), "voice_expand")
        return out

    def randn_rows(self, seeds, ns, steps: int, n_max: Optional[int] = None) -> torch.Tensor:
        """(steps, B, n_max, 64) sampler noise in one launch: row b of step s = randn(ns[b] * 64, seeds[b], s), zeros behind."""
        ns = [int(n) for n in ns]
        B = len(ns)
        Nm = max(ns) if n_max is None else int(n_max)
        if B == 0 or len(seeds) != B or min(ns) < 0 or max(ns) > Nm or Nm < 1 or steps < 1:
            raise ValueError(f"randn_rows: {len(seeds)} seeds for {B} rows of {ns} frames (n_max {Nm}, {steps} steps)")
        tab = self._upload_i64([np.asarray([int(s) & (2 ** 64 - 1) for s in seeds], np.uint64).view(np.int64), ns])
        out = torch.empty(int(steps), B, Nm, LATENT, device=self.device)
        self._ck(self.lib.smtts_randn_rows(self.h, self._stream(), _p(out), _p(tab[0]), _p(tab[1]), int(steps), B, Nm), "randn_rows")
        return out

    def stitch(self, audio: torch.Tensor, ns, offsets, fade: Optional[torch.Tensor], out: torch.Tensor) -> torch.Tensor:
        """Rows of a decoded batch into one waveform: audio (B,1,hop*Nmax) fp32 on the device, ns frames per row, offsets the rows'
        absolute sample offsets in `out` (1-D fp32 or int16 on the device, zero-filled once by the caller), fade the (F,) fp32
        weight table on the device or None.  out[offsets[b] + i] = audio[b, 0, i] * g for i < hop * ns[b] (smtts_stitch)."""
        B = audio.shape[0]
        row = int(audio.shape[-1])
        lens = [self.hop * int(n) for n in ns]
        if not self._is(audio, torch.float32) or len(lens) != B or len(offsets) != B or max(lens) > row:
            raise ValueError("stitch: audio must be contiguous fp32 (B,1,S) on the engine's device with hop * ns[b] <= S")
        out_1d("stitch", self.device, out)
        if any(int(o) < 0 or int(o) + n > out.numel() for o, n in zip(offsets, lens)):
            raise ValueError("stitch: a row does not fit into out")
        F = fade_len("stitch", self.device, fade)
        tab = self._upload_i64([lens, [int(o) for o in offsets]])
        self._ck(self.lib.smtts_stitch(self.h, self._stream(), _p(audio), B, row, _p(tab[0]), _p(tab[1]), _p(fade) if F else None, F,
                                       _p(out), out.numel(), int(out.dtype == torch.int16)), "stitch")
        return out

    def endpoints(self, audio: torch.Tensor, ns, ep, *, lens=None, return_peaks: bool = False):
        """Endpoints of the speech in each row of a decoded batch (smtts_endpoints; the definition: include/smalltts_hip.h).
        audio (B,1,S) contiguous fp32 on the device; ns frames per row (row b is its first hop * ns[b] samples), or `lens` samples
        per row instead (pass ns=None); ep an api.Endpointing (anything with .kernel_params()).  -> (seg, gain, e) on the device:
        seg int64 (B,2) = (start, n), gain fp32 (B), e fp32 (B, ceil(S / W)) the per-frame mean power (row b: ceil(len_b / W) entries, NOT written behind);
        with return_peaks=True also pk, the per-frame peaks.  Two launches on the current stream, no synchronisation."""
        if audio.dim() != 3 or audio.shape[1] != 1:
            raise ValueError("endpoints: audio must be (B,1,S)")
        B, row = int(audio.shape[0]), int(audio.shape[-1])
        if (ns is None) == (lens is None):
            raise ValueError("endpoints: pass either ns (frames per row) or lens= (samples per row)")
        lens = [self.hop * int(n) for n in ns] if lens is None else [int(n) for n in lens]
        if not self._is(audio, torch.float32) or B < 1 or row < 1 or len(lens) != B or min(lens) < 0 or max(lens) > row:
            raise ValueError("endpoints: audio must be contiguous fp32 (B,1,S) on the engine's device with 0 <= len[b] <= S")
        p = ep.kernel_params()
        W = int(p["W"])
        if W % 4 or not 16 <= W <= 4096 or not 1 <= int(p["min_run"]) <= 16 or int(p["lead"]) < 0 or int(p["tail"]) < 0:
            raise ValueError(f"endpoints: W % 4 == 0, 16 <= W <= 4096, 1 <= min_run <= 16, lead, tail >= 0 (got {p})")
        Fmax = (row + W - 1) // W
        e = torch.empty(2, B, Fmax, device=self.device)         # [0] mean power, [1] peak: no fill launch
        seg = torch.empty(B, 2, dtype=torch.int64, device=self.device)
        gain = torch.empty(B, device=self.device)
        tab = self._upload_i64([lens])
        self._ck(self.lib.smtts_endpoints(self.h, self._stream(), _p(audio), B, row, _p(tab[0]), W, float(p["rel_pow"]),
                                          float(p["floor_pow"]), int(p["min_run"]), int(p["lead"]), int(p["tail"]),
                                          float(p["target_rms"]), float(p["peak_limit"]), float(p["max_gain"]), _p(e[0]), _p(e[1]),
                                          _p(seg), _p(gain)), "endpoints")
        return (seg, gain, e[0], e[1]) if return_peaks else (seg, gain, e[0])

    def stitch_seg(self, audio: torch.Tensor, seg: torch.Tensor, gain: Optional[torch.Tensor], offsets, fade: Optional[torch.Tensor],
                   out: torch.Tensor) -> torch.Tensor:
        """stitch with a source window and an optional gain per row (smtts_stitch_seg): seg int64 (B,2) = (start, n) and gain fp32 (B)
        or None, both on the device as endpoints() returns them; offsets the windows' absolute sample offsets in `out` (host
        integers).  out[offsets[b] + i] = audio[b, 0, start_b + i] * gain[b] * g for i < n_b.  The windows are clamped into the row and
        samples outside `out` are dropped by the kernel: the host does not know n_b here."""
        B, row = int(audio.shape[0]), int(audio.shape[-1])
        if not self._is(audio, torch.float32) or len(offsets) != B or row < 1:
            raise ValueError("stitch_seg: audio must be contiguous fp32 (B,1,S) on the engine's device, one offset per row")
        seg_gain("stitch_seg", self.device, B, seg, gain)
        out_1d("stitch_seg", self.device, out)
        if out.numel() == 0:
            return out
        if any(int(o) < 0 or int(o) > out.numel() for o in offsets):
            raise ValueError("stitch_seg: an offset lies outside out")
        F = fade_len("stitch_seg", self.device, fade)
        tab = self._upload_i64([[int(o) for o in offsets]])
        self._ck(self.lib.smtts_stitch_seg(self.h, self._stream(), _p(audio), B, row, _p(seg), _p(gain), _p(tab[0]),
                                           _p(fade) if F else None, F, _p(out), out.numel(), int(out.dtype == torch.int16)), "stitch_seg")
        return out

    # ---- the running join: the joined stream handed out batch by batch (include/smalltts_hip.h smtts_join_stream) ----
    def join_state(self) -> torch.Tensor:
        """A zeroed join slot: int64 (2,) = (pos, k) on the device, the start of a joined stream.  state.clone() / .copy_() snapshot
        and rewind it."""
        return torch.zeros(2, dtype=torch.int64, device=self.device)

    def join_stream(self, audio: torch.Tensor, seg: torch.Tensor, gain: Optional[torch.Tensor], fade: Optional[torch.Tensor], gap: int,
                    state: torch.Tensor, *, last: bool, pcm16: bool, cap: Optional[int] = None, deliver_slot: Optional[int] = None):
        """The next pieces of a joined stream (smtts_join_stream): audio (B,1,S) fp32, seg int64 (B,2) = (start, n) and gain fp32 (B)
        or None on the device as endpoints() returns them, fade the (F,) fp32 table on the device or None, gap samples between
        non-empty pieces, state = join_state() carried from call to call.  -> (chunk, off, rec, dtable), all on the device: chunk
        (cap,) fp32 or int16 holds the stream's next rec[1] - rec[0] samples, off (B,) the pieces' absolute positions, rec (4,) =
        (pos before, pos after, k before, k after), dtable (4,) = (deliver_slot or 0, pos before, length, last), the row
        deliver_from_table reads.  cap defaults to B * (S + gap), which no table can overrun.  off, rec and dtable are views of ONE
        int64 tensor (chunk-independent), so a caller copies them out together.  On the current stream, no synchronisation."""
        if audio.dim() != 3 or audio.shape[1] != 1:
            raise ValueError("join_stream: audio must be (B,1,S)")
        B, row = int(audio.shape[0]), int(audio.shape[-1])
        if not self._is(audio, torch.float32) or B < 1 or row < 1:
            raise ValueError("join_stream: audio must be contiguous fp32 (B,1,S) on the engine's device")
        seg_gain("join_stream", self.device, B, seg, gain)
        F = fade_len("join_stream", self.device, fade)
        if not self._is(state, torch.int64, 2, aligned=True):
            raise ValueError("join_stream: state must be a contiguous, 16-byte aligned int64 (2,) tensor on the engine's device (join_state())")
        gap = int(gap)
        if gap < 0:
            raise ValueError("join_stream: gap must not be negative")
        cap = B * (row + gap) if cap is None else int(cap)
        if cap < 1:
            raise ValueError("join_stream: cap must be at least 1")
        chunk = torch.empty(cap, dtype=torch.int16 if pcm16 else torch.float32, device=self.device)
        small = torch.empty(B + 8, dtype=torch.int64, device=self.device)
        off, rec, dtable = small[:B], small[B: B + 4], small[B + 4:]
        self._ck(self.lib.smtts_join_stream(self.h, self._stream(), _p(audio), B, row, _p(seg), _p(gain), _p(fade) if F else None, F, gap,
                                            int(bool(last)), _p(state), _p(chunk), cap, int(bool(pcm16)), _p(off), _p(rec), _p(dtable),
                                            int(deliver_slot or 0)), "join_stream")
        return chunk, off, rec, dtable

    # ---- device-side audio front / back end ---------------------------------------------------------
    def resample(self, audio, sr: int, target: int = 24_000) -> torch.Tensor:
        """(samples,) or (channels, samples) float -> resampled on the device (same bank as audio.resample_hq)."""
        import math
        from .audio import _sinc_kernel
        x = self._dev(torch.as_tensor(audio, dtype=torch.float32), torch.float32)
        squeeze = x.dim() == 1
        if squeeze:
            x = x[None]
        x = x.contiguous()
        if sr == target:
            return x[0] if squeeze else x
        g = math.gcd(int(sr), int(target))
        down, up = sr // g, target // g
        key = (down, up)
        bank = self._banks.get(key)
        if bank is None:
            k, width = _sinc_kernel(down, up)
            bank = (torch.from_numpy(k).to(self.device).contiguous(), width)
            self._banks[key] = bank
        kern, width = bank
        n_in = x.shape[-1]
        n_out = int(math.ceil(up * n_in / down))
        y = torch.empty(x.shape[0], n_out, device=self.device)
        self._ck(self.lib.smtts_resample_poly(self.h, self._stream(), _p(x), x.shape[0], n_in, _p(kern), up, down,
                                              kern.shape[1], width, _p(y), n_out), "resample_poly")
        return y[0] if squeeze else y

    def pcm16(self, audio) -> torch.Tensor:
        """float [-1, 1] (any shape) -> int16 PCM on the device (clamp, x 32767, round to nearest)."""
        x = self._dev(torch.as_tensor(audio, dtype=torch.float32), torch.float32).contiguous()
        y = torch.empty(x.shape, dtype=torch.int16, device=self.device)
        self._ck(self.lib.smtts_pcm16(self.h, self._stream(), _p(x), x.numel(), _p(y)), "pcm16")
        return y

    # ---- delivery: audio at the caller's rate and encoding, whole or streamed (include/smalltts_hip.h smtts_deliver) ----
    def deliver_bank(self, rate: int, zeros: Optional[int] = None):
        """-> (bank (up, klen) fp32 on the device or None at 24 kHz, up, down, width, klen), cached per (rate, zeros)."""
        from .audio import DELIVER_ZEROS, _sinc_kernel, deliver_ratio
        up, down = deliver_ratio(rate)
        if (up, down) == (1, 1):
            return None, 1, 1, 0, 0
        zeros = DELIVER_ZEROS if zeros is None else int(zeros)
        key = ("deliver", int(rate), zeros)
        bank = self._banks.get(key)
        if bank is None:
            k, width = _sinc_kernel(down, up, zeros)
            bank = (torch.from_numpy(k).to(self.device).contiguous(), width)
            self._banks[key] = bank
        return bank[0], up, down, bank[1], int(bank[0].shape[1])

    def deliver_state(self, n_slots: int, rate: int, zeros: Optional[int] = None) -> Optional[torch.Tensor]:
        """A zeroed state pool of n_slots delivery streams at `rate`: uint8 (n_slots, smtts_deliver_state_bytes) on the device, the
        last klen - 1 input samples of each stream.  None at 24 kHz (the pass-through carries nothing).  A zero slot is the start of
        a stream; state[k].clone() / .copy_() snapshot and rewind it, like decode_state()."""
        if int(n_slots) < 1:
            raise ValueError("deliver_state: at least one slot")
        klen = self.deliver_bank(rate, zeros)[4]
        if klen == 0:
            return None
        sb = int(self.lib.smtts_deliver_state_bytes(self.h, klen))
        if sb <= 0:
            raise RuntimeError(f"deliver_state: {self.lib.smtts_last_error(self.h).decode()}")
        return torch.zeros(int(n_slots), sb, dtype=torch.uint8, device=self.device)

    def deliver(self, audio, lens, rate: int, encoding: str = "f32", *, state: Optional[torch.Tensor] = None, slots=None,
                n_before=None, last=True, zeros: Optional[int] = None, mark=None, mark_state: Optional[torch.Tensor] = None):
        """audio (B,1,S) fp32 on the device, row b = the next lens[b] samples of its stream -> (out (B, max count) in the encoding's
        dtype on the device, counts): row b of `out` holds counts[b] samples at `rate`, nothing is written behind them
        (smtts_deliver).  encoding "f32" | "pcm16" | "mulaw" | "alaw".  Whole signals: state=None (then n_before must be 0 and last
        True).  Streams: state=deliver_state(...), slots = B distinct slot indices, n_before = samples each stream has seen, last =
        True (or a flag per row) on a stream's final chunk; the chunks' concatenation is the whole call's result, bit for bit.
        counts come from audio.deliver_counts: integers alone.  The table goes up pinned and non-blocking; on the current stream, no
        synchronisation.
        mark = (key, strength) (or an object with .key and .strength): the 24 kHz rows are watermarked on the SAME table
        into a scratch buffer in front of smtts_deliver (engine.watermark's launches, nothing else changes).  mark_state =
        watermark_state(...) carries the mark from chunk to chunk through the same `slots` and `n_before`, also at 24 kHz, where the
        delivery itself has no state; without it every row starts a stream of its own."""
        from .audio import deliver_counts
        front = enc, bank, up, down, width, klen = self._deliver_front("deliver", rate, encoding, zeros, mark, mark_state)
        B, row, ln = self._audio_rows("deliver", audio, lens)
        lasts = [bool(v) for v in last] if isinstance(last, (list, tuple)) else [bool(last)] * B
        nb = [0] * B if n_before is None else [int(v) for v in n_before]
        if len(lasts) != B or len(nb) != B or min(nb) < 0:
            raise ValueError(f"deliver: one non-negative n_before and one last flag per row wanted, got {nb}, {lasts}")
        n_slots = self._deliver_pool("deliver", state, bank, klen)
        if state is not None:
            sl = distinct_slots("deliver", slots, B, n_slots)
        else:
            if (slots is not None and mark_state is None) or (bank is not None and (any(nb) or not all(lasts))):
                raise ValueError("deliver: without state every row starts and ends here: no slots, n_before = 0, last = True "
                                 "(24 kHz, a pure encode, takes any n_before and last and ignores them)")
            sl = [0] * B
        if mark_state is not None:
            sl = distinct_slots("deliver", slots, B, self._watermark_pool(mark_state, "deliver"))
        counts = list(ln) if bank is None else deliver_counts(nb, ln, lasts, up, down, width)
        tab = self._upload_i64([[s, a, n, int(f)] for s, a, n, f in zip(sl, nb, ln, lasts)])
        return self._deliver_table("deliver", audio, B, row, tab, front, state, n_slots, mark, mark_state), counts

    def _deliver_front(self, what, rate, encoding, zeros, mark, mark_state):
        """deliver / deliver_from_table: the encoding's code and the bank -> (enc, bank, up, down, width, klen)."""
        from .audio import DELIVER_ENCODINGS
        if mark is None and mark_state is not None:
            raise ValueError(f"{what}: mark_state= belongs to mark=")
        if encoding not in DELIVER_ENCODINGS:
            raise ValueError(f"{what}: encoding must be one of {DELIVER_ENCODINGS}, got {encoding!r}")
        return (DELIVER_ENCODINGS.index(encoding),) + tuple(self.deliver_bank(rate, zeros))

    def _deliver_pool(self, what, state, bank, klen) -> int:
        """The optional state pool of a delivery -> n_slots, 0 without one."""
        if state is None:
            return 0
        if bank is None:
            raise ValueError(f"{what}: 24 kHz is a pure encode and carries no state: pass state=None")
        return pool_slots(what, self.device, state, int(self.lib.smtts_deliver_state_bytes(self.h, klen)), "state", "deliver_state")

    def _deliver_table(self, what, audio, B, row, tab, front, state, n_slots, mark, mark_state) -> torch.Tensor:
        """The result, the mark and smtts_deliver on a table that lies on the device."""
        from .audio import deliver_max_count
        enc, bank, up, down, width, klen = front
        stride = row if bank is None else max(1, deliver_max_count(row, up, down, width, state is not None))
        out = torch.empty(B, stride, dtype=(torch.float32, torch.int16, torch.uint8, torch.uint8)[enc], device=self.device)
        if mark is not None:
            audio = self._watermark_table(audio, B, row, tab, mark, mark_state, what)
        self._ck(self.lib.smtts_deliver(self.h, self._stream(), _p(audio), B, row, _p(tab), _p(bank), up, down, klen, width, _p(state),
                                        n_slots, enc, _p(out), stride), "deliver")
        return out

    def deliver_from_table(self, chunk: torch.Tensor, dtable: torch.Tensor, rate: int, encoding: str = "f32", *,
                           state: Optional[torch.Tensor] = None, zeros: Optional[int] = None, mark=None,
                           mark_state: Optional[torch.Tensor] = None) -> torch.Tensor:
        """deliver() for ONE row whose table row already lies on the device: chunk (cap,) fp32 and dtable int64 (4,) = (slot, n_before,
        len, last) as join_stream() wrote them, so the delivery is enqueued right behind the join without the host knowing the
        length.  -> out (1, audio.deliver_max_count(cap, ...)) in the encoding's dtype on the device; the row's count follows
        afterwards from join_stream's rec with audio.deliver_counts(rec[0], rec[1] - rec[0], last, up, down, width): integers alone
        (at 24 kHz: rec[1] - rec[0]).  state = deliver_state(...) carries the stream from chunk to chunk through the slot dtable names
        (clamped into the pool by the kernel); state=None: the chunk starts and ends a stream of its own (at 24 kHz, a pure encode,
        there is nothing to carry and state must be None).  On the current stream, no synchronisation.
        mark / mark_state: as in deliver(): the chunk is watermarked on the device-written dtable in front of smtts_deliver, so the
        mark follows the stream's absolute position without the host knowing the length."""
        front = enc, bank, up, down, width, klen = self._deliver_front("deliver_from_table", rate, encoding, zeros, mark, mark_state)
        if not self._is(chunk, torch.float32, None) or int(chunk.numel()) < 1:
            raise ValueError("deliver_from_table: chunk must be a contiguous 1-D fp32 tensor on the engine's device")
        if not self._is(dtable, torch.int64, 4):
            raise ValueError("deliver_from_table: dtable must be a contiguous int64 (4,) tensor on the engine's device")
        n_slots = self._deliver_pool("deliver_from_table", state, bank, klen)
        if mark_state is not None:
            self._watermark_pool(mark_state, "deliver_from_table")
        return self._deliver_table("deliver_from_table", chunk, 1, int(chunk.numel()), dtable, front, state, n_slots, mark, mark_state)

    # ---- watermark: key the 24 kHz stream, detect it (include/smalltts_hip.h smtts_watermark) ----
    @staticmethod
    def _mark_pair(mark, what: str):
        """mark= -> (key as uint64, strength)."""
        key, strength = (mark.key, mark.strength) if hasattr(mark, "key") else tuple(mark)
        key, strength = int(key), float(strength)
        if not 0 <= key < 2 ** 64:
            raise ValueError(f"{what}: the key must be in [0, 2^64), got {key}")
        if not (0.0 <= strength <= 1.0):
            raise ValueError(f"{what}: strength must be in [0, 1], got {strength}")
        return key, strength

    def watermark_state(self, n_slots: int) -> torch.Tensor:
        """A zeroed state pool of n_slots watermark streams: uint8 (n_slots, smtts_watermark_state_bytes) on the device, the last 127
        unmarked samples of each stream.  A zero slot is the start of a stream; state[k].clone() / .copy_() snapshot and rewind it."""
        if int(n_slots) < 1:
            raise ValueError("watermark_state: at least one slot")
        return torch.zeros(int(n_slots), int(self.lib.smtts_watermark_state_bytes(self.h)), dtype=torch.uint8, device=self.device)

    def _watermark_pool(self, state, what: str) -> int:
        return pool_slots(what, self.device, state, int(self.lib.smtts_watermark_state_bytes(self.h)), "the mark state", "watermark_state")

    def _audio_rows(self, what, audio, lens):
        """deliver / watermark: audio fp32 (B,1,S) and its B lengths -> (B, S, the lengths as ints)."""
        if not self._is(audio, torch.float32, None, 1, None) or int(audio.shape[0]) < 1 or int(audio.shape[2]) < 1:
            raise ValueError(f"{what}: audio must be a contiguous fp32 (B,1,S) tensor on the engine's device with B, S >= 1")
        B, row = int(audio.shape[0]), int(audio.shape[2])
        return B, row, row_lengths(what, lens, B, row)

    def _watermark_table(self, audio: torch.Tensor, B: int, row: int, tab: torch.Tensor, mark, state, what: str) -> torch.Tensor:
        """smtts_watermark on a table that already lies on the device -> the marked copy, shaped like audio."""
        key, strength = self._mark_pair(mark, what)
        out = torch.empty_like(audio)
        self._ck(self.lib.smtts_watermark(self.h, self._stream(), _p(audio), B, row, _p(tab), key, strength, _p(state),
                                          0 if state is None else int(state.shape[0]), _p(out)), "watermark")
        return out

    def watermark(self, audio, lens, key: int, strength: float = 0.02, *, state: Optional[torch.Tensor] = None, slots=None,
                  n_before=None) -> torch.Tensor:
        """audio (B,1,S) fp32 on the device, row b = the next lens[b] samples of its 24 kHz stream -> the marked copy (B,1,S): row b
        holds lens[b] marked samples, nothing is written behind them (smtts_watermark).  Whole signals: state=None (every row starts
        a stream).  Streams: state=watermark_state(...), slots = B distinct slot indices, n_before = samples each stream has seen;
        the chunks' concatenation is the whole call's result, bit for bit.  On the current stream, no synchronisation."""
        B, row, ln = self._audio_rows("watermark", audio, lens)
        nb = [0] * B if n_before is None else [int(v) for v in n_before]
        if len(nb) != B or min(nb) < 0:
            raise ValueError(f"watermark: one non-negative n_before per row wanted, got {nb}")
        if state is not None:
            sl = distinct_slots("watermark", slots, B, self._watermark_pool(state, "watermark"))
        else:
            if slots is not None or any(nb):
                raise ValueError("watermark: without state every row starts here: no slots, n_before = 0")
            sl = [0] * B
        tab = self._upload_i64([[s, a, n, 0] for s, a, n in zip(sl, nb, ln)])
        return self._watermark_table(audio, B, row, tab, (key, strength), state, "watermark")

    def watermark_detect(self, audio: torch.Tensor, lens, key: int, *, o_lo: int = 0, n_off: int = 1, return_u: bool = False):
        """audio fp32 (B,S) on the device, row b = lens[b] samples at 24 kHz -> (T (B,n_off), den (B), best_off (B) int64, best_z (B)[,
        u (B,S)]) on the device (smtts_watermark_detect): T[b][k] is the sign correlation at offset o_lo + k ("audio[j] is stream
        sample j + o"), best_off = o_lo + argmax, best_z = T / sqrt(den), about N(0, 1) where the key's mark is absent.  u is written
        below lens[b] only (zeros behind).  Needs no weights.  Three launches on the current stream, no synchronisation."""
        if not self._is(audio, torch.float32, None, None) or not 1 <= int(audio.shape[0]) <= 1024 or int(audio.shape[1]) < 1:
            raise ValueError("watermark_detect: audio must be a contiguous fp32 (B,S) tensor on the engine's device, 1 <= B <= 1024, S >= 1")
        B, row = int(audio.shape[0]), int(audio.shape[1])
        ln = row_lengths("watermark_detect", lens, B, row)
        key, o_lo, n_off = int(key), int(o_lo), int(n_off)
        if not 0 <= key < 2 ** 64:
            raise ValueError(f"watermark_detect: the key must be in [0, 2^64), got {key}")
        if not (0 <= o_lo <= 2 ** 40 and 1 <= n_off <= 65536):
            raise ValueError(f"watermark_detect: o_lo in [0, 2^40] and n_off in [1, 65536] wanted, got {o_lo}, {n_off}")
        need = int(self.lib.smtts_watermark_detect_workspace_bytes(self.h, B, row))
        if need <= 0:
            raise RuntimeError(f"watermark_detect: {self.lib.smtts_last_error(self.h).decode()}")
        ws = self._workspace(need)
        u = torch.zeros(B, row, device=self.device) if return_u else None
        T = torch.empty(B, n_off, device=self.device)
        den = torch.empty(B, device=self.device)
        best_z = torch.empty(B, device=self.device)
        best_off = torch.empty(B, dtype=torch.int64, device=self.device)
        lens_d = self._upload_i64(ln)
        self._ck(self.lib.smtts_watermark_detect(self.h, self._stream(), _p(audio), B, row, _p(lens_d), key, o_lo, n_off, _p(ws), need,
                                                 _p(u), _p(den), _p(T), _p(best_off), _p(best_z)), "watermark_detect")
        return (T, den, best_off, best_z, u) if return_u else (T, den, best_off, best_z)

    # ---- retiming: WSOLA onto a table of anchors (include/smalltts_hip.h smtts_retime) ----
    def retime(self, audio: torch.Tensor, lens, anchors, *, hop: int = 240, delta: int = 120, return_q: bool = False):
        """audio (B,1,S) fp32 on the device, row b = lens[b] samples at 24 kHz; anchors: per row one integer array (m_b, 2) = (src,
        dst) on the host (plans.retime_anchors) -> (out (B,1,S_out) fp32 on the device, out_lens[, q]): row b holds out_lens[b] =
        its last dst samples, zeros behind; S_out is the largest of them.  q int64 (B, ceil(S_out / hop)): the source position every
        segment was taken from (row b: ceil(out_lens[b] / hop) entries, zeros behind).  A table starts at dst 0, src and dst
        increase strictly, 0 <= src <= lens[b], and between two anchors the source runs at 1/8 to 8 times the output's speed.
        One launch on the current stream, no synchronisation."""
        B, row, ln = self._audio_rows("retime", audio, lens)
        hop, delta = int(hop), int(delta)
        if B > 1024 or row > 2 ** 31 - 1:
            raise ValueError(f"retime: at most 1024 rows of at most 2^31 - 1 samples, got {B} x {row}")
        if not 16 <= hop <= 512 or hop % 4 or not 0 <= delta <= 512:
            raise ValueError(f"retime: hop a multiple of 4 in [16, 512] and delta in [0, 512] wanted, got {hop}, {delta}")
        if len(anchors) != B:
            raise ValueError(f"retime: one anchor table per row wanted, got {len(anchors)} for {B} rows")
        tabs = [np.asarray(a) for a in anchors]
        for b, a in enumerate(tabs):
            if a.ndim != 2 or a.shape[1] != 2 or not 2 <= a.shape[0] <= 65536 or a.dtype.kind not in "iu":
                raise ValueError(f"retime: anchors[{b}] must be an integer (m, 2) array of (src, dst) with 2 <= m <= 65536, got "
                                 f"{a.dtype} {a.shape}")
        tabs = [a.astype(np.int64) for a in tabs]
        for b, a in enumerate(tabs):
            ds, dd = np.diff(a[:, 0]), np.diff(a[:, 1])
            if a[0, 1] != 0:
                raise ValueError(f"retime: anchors[{b}] must start at dst 0, got {int(a[0, 1])}")
            if (ds <= 0).any() or (dd <= 0).any():
                raise ValueError(f"retime: src and dst of anchors[{b}] must both increase strictly")
            if a[0, 0] < 0 or a[-1, 0] > ln[b]:
                raise ValueError(f"retime: src of anchors[{b}] must lie in [0, {ln[b]}], got [{int(a[0, 0])}, {int(a[-1, 0])}]")
            if (ds > 8 * dd).any() or (dd > 8 * ds).any():
                raise ValueError(f"retime: between two anchors of anchors[{b}] the source must run at 1/8 to 8 times the output's speed")
            if a[-1, 1] > 2 ** 31 - 1:
                raise ValueError(f"retime: anchors[{b}] ends behind 2^31 - 1 output samples")
        A = max(a.shape[0] for a in tabs)
        out_lens = [int(a[-1, 1]) for a in tabs]
        S_out = max(out_lens)
        padded = np.zeros((B, A, 2), np.int64)
        for b, a in enumerate(tabs):
            padded[b, :a.shape[0]] = a
        tab = self._upload_i64(np.concatenate([np.asarray(ln, np.int64), np.asarray([a.shape[0] for a in tabs], np.int64),
                                               padded.reshape(-1)]))
        win = self._retime_wins.get(hop)
        if win is None:
            win = self._retime_wins[hop] = torch.from_numpy(retime_window(hop)).to(self.device)
        out = torch.zeros(B, 1, S_out, device=self.device)     # a row's tail behind its own length is not written by the kernel
        q = torch.zeros(B, (S_out + hop - 1) // hop, dtype=torch.int64, device=self.device) if return_q else None
        self._ck(self.lib.smtts_retime(self.h, self._stream(), _p(audio), B, row, _p(tab[:B]), _p(tab[2 * B:]), _p(tab[B: 2 * B]), A,
                                       _p(win), hop, delta, _p(out), S_out, _p(q)), "retime")
        return (out, out_lens, q) if return_q else (out, out_lens)

    # ---- pitch: NCCF scores and the best path through them (include/smalltts_hip.h smtts_pitch) ----
    def pitch(self, audio: torch.Tensor, lens, pitch=None, return_nccf: bool = False):
        """audio (B,1,S) fp32 on the device, row b = lens[b] samples at 24 kHz; pitch: an options.Pitch (None: its defaults) -> (lag
        (B,Fmax) int32, peak (B,Fmax,3) fp32[, nccf (B,Fmax,L) fp32]) on the device, Fmax = ceil(S / hop): lag is 0 where a frame is
        unvoiced, else its period in samples; peak holds the score at the lag and at its two neighbours (plans.pitch_f0 makes f0 and
        strength of the two).  Row b holds ceil(lens[b] / hop) frames, zeros behind.  Two launches on the current stream, no
        synchronisation.  Checked on synthetic signals only, not on speech."""
        B, row, ln = self._audio_rows("pitch", audio, lens)
        pt = as_pitch(pitch)
        if B > 1024 or row > 2 ** 24:
            raise ValueError(f"pitch: at most 1024 rows of at most 2^24 samples, got {B} x {row}")
        need = int(self.lib.smtts_pitch_workspace_bytes(self.h, B, row, pt.hop, pt.lmin, pt.lmax))
        if need <= 0:
            raise RuntimeError(f"pitch: {self.lib.smtts_last_error(self.h).decode()}")
        ws = self._workspace(need)
        key = (pt.lmin, pt.lmax, pt.tilt)
        tab = self._pitch_tabs.get(key)
        if tab is None:
            tab = self._pitch_tabs[key] = torch.from_numpy(pitch_tables(*key)).to(self.device)
        Fmax, L = (row + pt.hop - 1) // pt.hop, pt.lmax - pt.lmin + 1
        lag = torch.zeros(B, Fmax, dtype=torch.int32, device=self.device)   # a row's frames behind its own length are not written
        peak = torch.zeros(B, Fmax, 3, device=self.device)
        nccf = torch.zeros(B, Fmax, L, device=self.device) if return_nccf else None
        lens_d = self._upload_i64(ln)
        self._ck(self.lib.smtts_pitch(self.h, self._stream(), _p(audio), B, row, _p(lens_d), _p(tab), pt.hop, pt.win, pt.lmin, pt.lmax,
                                      pt.bias, pt.c_unv, pt.w_jump, pt.w_switch, _p(lag), _p(peak), _p(nccf), _p(ws), need), "pitch")
        return (lag, peak, nccf) if return_nccf else (lag, peak)

    def profile(self, on, tagged: bool = False, shapes: bool = False):
        """on: False/True; tagged=True prefixes kernel names with the pipeline phase (enc, mod, dit, dec.s<i> ...); shapes=True
        (implies tagged) also appends each GEMM product's shape to its class name ("gemm3<...> 600x3840x960").
        Works under either tuning (bench.py profiles the throughput-tuned kernels it times) but only ONE call at a time: the
        named per-batch workspaces of batches in flight are refused while it is on."""
        if on and self._ws_slot is not None:
            raise RuntimeError("per-kernel profiling pairs HIP events around every launch and assumes ONE call at a time: "
                               "finish the batches in flight (use_workspace(None)) first")
        self._profiling = bool(on)
        self._ck(self.lib.smtts_profile_enable(self.h, (3 if shapes else 2 if tagged else 1) if on else 0), "profile_enable")

    def profile_report(self):
        import json
        buf = C.create_string_buffer(1 << 20)
        self._ck(self.lib.smtts_profile_report(self.h, buf, len(buf)), "profile_report")
        return json.loads(buf.value.decode())

    def alpha_sigma(self, t: float):
        a, s = C.c_float(), C.c_float()
        self.lib.smtts_alpha_sigma(C.c_float(t), C.byref(a), C.byref(s))
        return a.value, s.value
