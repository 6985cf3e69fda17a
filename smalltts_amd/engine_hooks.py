"""The single-kernel test hooks of HipEngine: the host twin of csrc/engine_hooks.hip.  No product path calls them; HipEngine inherits
this mixin, so tests/ and tools/ find them where they always were.  It uses the engine's lib, h, device, precision, _ck, _dev, _stream
and set_precision."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from ._lib import ACT, PRECISION, SITES, ptr as _p
from .weights import HEAD_DIM, LATENT_DIM as LATENT, N_BLOCKS as N_LAYERS, N_HEADS


SCORER_NETS = {"asr": 0, "sv": 1}
_ASR_LAYER = ("ffn1", "qkv", "attn", "proj", "conv", "ffn2")
_SV_BLOCK = ("tdnn1", "res2net", "tdnn2", "gate", "out")
# the slots of smtts_test_scorer_taps: one per launch, in launch order
SCORER_TAPS = {
    "asr": ["upsample"] + [f"layers.{l}.{s}" for l in range(7) for s in _ASR_LAYER] + ["logp"],
    "sv": ["blocks.0"] + [f"blocks.{i}.{s}" for i in (1, 2, 3) for s in _SV_BLOCK] + ["mfa", "stats", "crow", "att", "logit", "pooled", "emb"],
}


def scorer_tap_shapes(net: str, B: int, N: int) -> Dict[str, tuple]:
    """the fp32 shape of every slot of SCORER_TAPS[net]"""
    if net == "asr":
        T = 4 * N
        return {n: (B, T, 198) if n == "logp" else (B, T, 192) if n.endswith(".qkv") else (B, T, 64) for n in SCORER_TAPS[net]}
    row = {"stats": 4608, "crow": 192, "pooled": 4608, "emb": 192}
    frame = {"mfa": 2304, "att": 192, "logit": 2304}
    return {n: (B, row[n]) if n in row else (B, 768) if n.endswith(".gate") else (B, N, frame.get(n, 768)) for n in SCORER_TAPS[net]}


class EngineHooks:
    def set_ln_fold(self, on: bool) -> bool:
        """Test hook: the fused sampler's AdaLN between two DiT block GEMMs folded into their epilogues (default) or as separate
        split-K reduce / ln_modulate launches.  Returns the previous setting."""
        prev = self.ln_fold
        self._ck(self.lib.smtts_test_set_ln_fold(self.h, int(bool(on))), "test_set_ln_fold")
        self.ln_fold = bool(on)
        return prev

    def _f32(self, *ts):
        """the optional fp32 operands of a hook, on the device"""
        return [None if t is None else self._dev(t, torch.float32) for t in ts]

    def _test_gemm(self, entry, A, W, bias, act, split, cfg):
        """test_gemm / test_gemm3: the strided entry takes A's and the result's leading dimensions as well."""
        A, W, bias = self._f32(A, W, bias)
        M, K = A.shape
        N = W.shape[0]
        out = torch.empty(M, N, device=self.device)
        lda, ldc = ((K,), (N,)) if entry == "test_gemm" else ((), ())
        self._ck(getattr(self.lib, "smtts_" + entry)(self.h, self._stream(), _p(A), *lda, _p(W), _p(bias), M, N, K, ACT[act], split, cfg,
                                                     _p(out), *ldc), entry)
        return out

    def test_gemm(self, A, W, bias=None, act="none", split=3, cfg=-1):
        return self._test_gemm("test_gemm", A, W, bias, act, split, cfg)

    def test_gemm3(self, A, W, bias=None, act="none", split=3, cfg=-1):
        return self._test_gemm("test_gemm3", A, W, bias, act, split, cfg)

    def test_ln_fold(self, x, A, Wp, scale, W1, W3, shift=None, bp=None, gate=None, row_mask=None, b1=None, b3=None,
                     rms=False, fold=True, precision="f16", eps=1e-6, return_shift=False):
        """One LN-fold step (include/smalltts_hip.h smtts_test_ln_fold): x += row_mask gate (A Wp^T + bp), then the LayerNorm
        (1 + scale) + shift (rms=False) or RMSNorm * scale (rms=True) of x into [W1 | W3] and SwiGLU.  fold=True: the producer /
        consumer epilogues; False: the norm launches.  Returns (updated x [M, D], hidden [M, F]) as fp32, and with return_shift=True
        the row shift the consumer leaves for the next producer [M] (LayerNorm fold; zeros otherwise); x itself is not modified."""
        A, Wp, scale, W1, W3, shift, bp, gate, b1, b3 = self._f32(A, Wp, scale, W1, W3, shift, bp, gate, b1, b3)
        x = self._dev(x, torch.float32).clone()
        row_mask = None if row_mask is None else self._dev(row_mask, torch.uint8)
        M, K = A.shape
        D, F = Wp.shape[0], W1.shape[0]
        hid = torch.empty(M, F, device=self.device)
        shift_out = torch.empty(M, device=self.device) if return_shift else None
        self._ck(self.lib.smtts_test_ln_fold(self.h, self._stream(), _p(A), _p(Wp), _p(bp), _p(gate), _p(row_mask), _p(scale),
                                             _p(shift), _p(W1), _p(W3), _p(b1), _p(b3), M, K, D, F, eps, int(bool(rms)),
                                             PRECISION[precision], int(bool(fold)), _p(x), _p(hid), _p(shift_out)), "test_ln_fold")
        return (x, hid, shift_out) if return_shift else (x, hid)

    def test_codec_stage(self, part, stage: int, what: int, x) -> torch.Tensor:
        """One codec stage through the product's code (include/smalltts_hip.h smtts_test_codec_stage).  part: "decoder" / "encoder"
        (or 1 / 2); what: 1 stem, 2 resampling into `stage`, 4 its blocks, 8 final norm + head (a run of these bits).  x: (B, T_in, C_in)
        channels-last (encoder stem: (B, S) or (B, S, 1) audio).  Returns the device tensor (B, T_out, C_out); the decoder head's
        audio comes back as (B, T_out, 1)."""
        p = {"decoder": 1, "encoder": 2}.get(part, part)
        x = self._dev(x, torch.float32)
        if x.dim() == 2:
            x = x[:, :, None].contiguous()
        B, T, Cin = x.shape
        t_out, c_out = C.c_int(0), C.c_int(0)
        self._ck(self.lib.smtts_test_codec_stage(self.h, self._stream(), int(p), int(stage), int(what), _p(x), B, T, Cin, None,
                                                 C.byref(t_out), C.byref(c_out)), "test_codec_stage")
        out = torch.empty(B, t_out.value, c_out.value, device=self.device)
        self._ck(self.lib.smtts_test_codec_stage(self.h, self._stream(), int(p), int(stage), int(what), _p(x), B, T, Cin, _p(out),
                                                 C.byref(t_out), C.byref(c_out)), "test_codec_stage")
        return out

    def test_dit_stage(self, net: str, what: int, x=None, mask=None, l0: int = 0, l1: Optional[int] = None, path: str = "auto",
                       twice: bool = False, t=None, mod=None, mod_row0: int = 0, mod_rstride: int = 0, k_ref=None, v_ref=None,
                       ref_mask=None, k_text=None, v_text=None, ph_mask=None, rope=None) -> Dict[str, torch.Tensor]:
        """DiT / condition-encoder stages through the product's code (include/smalltts_hip.h smtts_test_dit_stage).  net: "dit", "style"
        or "text"; what: a run of the chain bits (DiT: 1 modulation from t, 2 embed, 4 blocks [l0, l1), 8 head; encoders: 1 input,
        2 blocks, 4 output projection, 8 cross K / V).  path: "auto" (the operator's choice), "fold", "splitk" or "unsplit".
        Returns the device tensors that apply: "x" residual, "img" the operand image the blocks leave (fp32), "shift" the fold's
        row shift, "out" velocity / ref_seq / phoneme memory, "k" / "v", "mod" the modulation table."""
        netc = {"dit": 0, "style": 1, "text": 2}[net]
        pathc = {"auto": 0, "fold": 1, "splitk": 2, "unsplit": 3}[path]
        if x is not None:
            x = self._dev(x, torch.int64 if (net == "text" and what & 1) else torch.float32)
            B, S = x.shape[:2]
        else:
            B, S = 1, 1
        if mask is not None:
            mask = self._dev(mask, torch.bool)
            B, S = mask.shape
        t, mod, k_ref, v_ref, k_text, v_text, rope = self._f32(t, mod, k_ref, v_ref, k_text, v_text, rope)
        ref_mask = None if ref_mask is None else self._dev(ref_mask, torch.bool)
        ph_mask = None if ph_mask is None else self._dev(ph_mask, torch.bool)
        rows = t.shape[0] if t is not None else mod.shape[0] if mod is not None else 0
        R = 0 if k_ref is None else k_ref.shape[3]
        P = 0 if k_text is None else k_text.shape[3]
        dit = net == "dit"
        D = 960 if dit else 512
        if l1 is None:
            l1 = N_LAYERS if net != "text" else 8
        e = lambda *sh: torch.empty(*sh, device=self.device)
        res: Dict[str, torch.Tensor] = {}
        if what & (6 if dit else 3):
            res["x"] = e(B, S, D)
        if what & (4 if dit else 2):
            res["img"] = e(B, S, D)
            if dit:
                res["shift"] = e(B, S)
        if dit and what & 8:
            res["out"] = e(B, S, LATENT)
        if not dit and what & 4:
            res["out"] = e(B, S, 960)
        if not dit and what & 8:
            res["k"], res["v"] = e(N_LAYERS, B, N_HEADS, S, HEAD_DIM), e(N_LAYERS, B, N_HEADS, S, HEAD_DIM)
        if dit and what & 1:
            res["mod"] = e(rows, 71040)
        self._ck(self.lib.smtts_test_dit_stage(self.h, self._stream(), netc, int(what), int(l0), int(l1), pathc, int(bool(twice)),
                                               _p(x), _p(mask), B, S, _p(t), _p(mod), rows, int(mod_row0), int(mod_rstride),
                                               _p(k_ref), _p(v_ref), _p(ref_mask), R, _p(k_text), _p(v_text), _p(ph_mask), P, _p(rope),
                                               _p(res.get("x")), _p(res.get("img")), _p(res.get("shift")), _p(res.get("out")),
                                               _p(res.get("k")), _p(res.get("v")), _p(res.get("mod"))), "test_dit_stage")
        return res

    def test_scorer_tap_slots(self, net: str, B: int, N: int):
        """-> (byte offset of every slot of smtts_test_scorer_taps, the tap buffer's size in bytes)"""
        off = (C.c_size_t * len(SCORER_TAPS[net]))()
        total = int(self.lib.smtts_test_scorer_tap_bytes(self.h, SCORER_NETS[net], int(B), int(N), off, len(off)))
        if not total:
            self._ck(1, "test_scorer_tap_bytes")
        return list(off), total

    def test_scorer_taps(self, net: str, x, ns) -> Dict[str, torch.Tensor]:
        """Every launch of one scorer call, tapped (include/smalltts_hip.h smtts_test_scorer_taps).  net: "asr" or "sv"; x fp32
        (B, N, 64), ns the rows' lengths.  -> {slot name of SCORER_TAPS[net]: the buffer that launch wrote, a device tensor}; the last
        slot is the call's result.  Elements nobody wrote (at and behind a row's length) are NaN."""
        x = self._dev(x, torch.float32)
        B, N = x.shape[:2]
        n_len = self._dev(torch.as_tensor([int(v) for v in ns], dtype=torch.int32), torch.int32)
        off, total = self.test_scorer_tap_slots(net, B, N)
        names = SCORER_TAPS[net]
        shapes = scorer_tap_shapes(net, B, N)
        buf = torch.empty(total, dtype=torch.uint8, device=self.device)
        out = torch.empty(shapes[names[-1]], device=self.device)
        self._ck(self.lib.smtts_test_scorer_taps(self.h, self._stream(), SCORER_NETS[net], _p(x), _p(n_len), B, N, _p(out), _p(buf),
                                                 total), "test_scorer_taps")
        res = {}
        for name, o in zip(names, off):
            sh = shapes[name]
            nb = 4 * int(torch.Size(sh).numel())
            res[name] = buf[o:o + nb].view(torch.float32).view(sh)
        return res

    def test_swiglu(self, A, W1, W3, b1=None, b3=None, split=3):
        A, W1, W3, b1, b3 = self._f32(A, W1, W3, b1, b3)
        M, K = A.shape
        F = W1.shape[0]
        out = torch.empty(M, F, device=self.device)
        self._ck(self.lib.smtts_test_swiglu(self.h, self._stream(), _p(A), _p(W1), _p(W3), _p(b1), _p(b3), M, F, K,
                                            split, _p(out)), "test_swiglu")
        return out

    def _test_attn(self, entry, what, fmt, qkvg, qw, kw, eps, rope, rot_dim, H, dh, k_ref, v_ref, k_text, v_text, mask_self, mask_ref,
                   mask_text):
        """The two attention hooks: the operands onto the device, the result, smtts_<entry>.  fmt: the precision the attention site
        runs the call at, or None; the engine's own comes back whether or not the call raises."""
        mass = what == "test_attn_text_mass"
        qkvg = self._dev(qkvg, torch.float32)
        B, N, _ = qkvg.shape
        qw, kw, rope, k_ref, v_ref, k_text, v_text = self._f32(qw, kw, rope, k_ref, v_ref, k_text, v_text)
        mask_self, mask_ref, mask_text = (None if m is None else self._dev(m, torch.bool) for m in (mask_self, mask_ref, mask_text))
        if mass and k_text is None:
            raise ValueError("test_attn_text_mass: needs text keys")
        R = 0 if k_ref is None else k_ref.shape[2]
        P = 0 if k_text is None else k_text.shape[2]
        out = torch.empty(B, N, P if mass else H * dh, device=self.device)
        if fmt is not None:
            self._ck(self.lib.smtts_set_site_precision(self.h, SITES["attn"], PRECISION[fmt]), "set_site_precision")
        try:
            self._ck(getattr(self.lib, "smtts_" + entry)(self.h, self._stream(), _p(qkvg), _p(qw), _p(kw), eps, _p(rope), rot_dim, _p(k_ref),
                                                         _p(v_ref), R, _p(k_text), _p(v_text), P, _p(mask_self), _p(mask_ref), _p(mask_text),
                                                         B, N, H, dh, _p(out)), what)
        finally:
            if fmt is not None:
                self.set_precision(self.precision)
        return out

    def test_attention(self, qkvg, qw, kw, eps, rope, rot_dim, H, dh, k_ref=None, v_ref=None, k_text=None, v_text=None,
                       mask_self=None, mask_ref=None, mask_text=None, mfma=False):
        """mfma: "img" / "img:f16" / "img:bf16x3" / "img:bf16": the product's DMA + MFMA kernel on operand images at that precision."""
        s = str(mfma)
        fmt = (s.split(":")[1] if ":" in s else "bf16x3") if mfma else None
        return self._test_attn("test_attention_mfma" if mfma else "test_attention", "test_attention", fmt, qkvg, qw, kw, eps, rope, rot_dim,
                               H, dh, k_ref, v_ref, k_text, v_text, mask_self, mask_ref, mask_text)

    def test_attn_text_mass(self, qkvg, qw, kw, eps, rope, rot_dim, H, dh, k_ref=None, v_ref=None, k_text=None, v_text=None,
                            mask_self=None, mask_ref=None, mask_text=None, fmt: str = "bf16x3"):
        """The text-attention tap in isolation (smtts_test_attn_text_mass): the inputs of test_attention(mfma="img:<fmt>"), the same
        operand images; -> mass fp32 (B,N,P), the mean over all heads of the softmax probability on each text key."""
        return self._test_attn("test_attn_text_mass", "test_attn_text_mass", fmt, qkvg, qw, kw, eps, rope, rot_dim, H, dh, k_ref, v_ref,
                               k_text, v_text, mask_self, mask_ref, mask_text)
