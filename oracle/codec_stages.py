"""ORACLE (test infrastructure, NOT product code): the codec of `oracle/codec_oracle.py` cut into the stages the engine runs one
at a time (smtts_test_codec_stage), written out in plain fp64 torch on channels-last (B, T, C) tensors.

Each operation is spelled out from its definition — causal windows as explicit frame shifts, ConvTranspose1d(k = 2r, stride r)
with its causal trim as the two taps each output frame receives, RMSNorm over channels, exact-erf GELU — instead of torch's conv
ops, so that it is a second formulation of what codec_oracle states.  Absent optional tensors take their identity value (bias 0,
layer scale 1, no final norm).  tests/test_codec_oracle.py pins the composition of these stages to codec_oracle.decode / encode."""
from __future__ import annotations

import math
from typing import Dict

import torch

from smalltts_amd.weights import CodecSpec

W = Dict[str, torch.Tensor]
DEC, ENC = "codec.decoder", "codec.encoder"


def f64(w: W) -> W:
    return {k: torch.as_tensor(v).to(torch.float64) for k, v in w.items()}


def _shift(x: torch.Tensor, s: int) -> torch.Tensor:
    """x delayed by s frames along T (zeros enter at the start): y[:, t] = x[:, t - s]."""
    if s == 0:
        return x
    T = x.shape[1]
    z = x.new_zeros(x.shape[0], min(s, T), x.shape[2])
    return torch.cat([z, x[:, : T - s]], 1) if s < T else z[:, :T]


def causal_conv(x: torch.Tensor, w: torch.Tensor, b=None, stride: int = 1) -> torch.Tensor:
    """Conv1d with left pad k - stride: x (B, T, Cin), w (Cout, Cin, k) -> (B, T // stride, Cout);
    out[t] = sum_j w[:, :, j] x[t stride + j - (k - stride)]."""
    k = w.shape[-1]
    To = x.shape[1] // stride
    xp = torch.cat([x.new_zeros(x.shape[0], k - stride, x.shape[2]), x], 1)
    y = sum(xp[:, j : j + To * stride : stride] @ w[:, :, j].t() for j in range(k))
    return y if b is None else y + b


def depthwise_conv(x: torch.Tensor, w: torch.Tensor, b=None) -> torch.Tensor:
    """causal depthwise conv: x (B, T, C), w (C, k): out[t, c] = sum_j w[c, j] x[t - (k - 1) + j, c]."""
    k = w.shape[-1]
    y = sum(_shift(x, k - 1 - j) * w[:, j] for j in range(k))
    return y if b is None else y + b


def conv_transpose(x: torch.Tensor, w: torch.Tensor, b, r: int) -> torch.Tensor:
    """ConvTranspose1d(k = 2r, stride r) trimmed to T r frames: x (B, T, Cin), w (Cin, Cout, 2r) -> (B, T r, Cout);
    out[q r + j] = x[q] w[:, :, j] + x[q - 1] w[:, :, j + r]."""
    B, T, _ = x.shape
    xp = _shift(x, 1)
    y = torch.stack([x @ w[:, :, j] + xp @ w[:, :, j + r] for j in range(r)], 2)   # (B, T, r, Cout)
    y = y.reshape(B, T * r, w.shape[1])
    return y if b is None else y + b


def rms(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * w


def gelu(h: torch.Tensor) -> torch.Tensor:
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def _scale(w: W, name: str, y: torch.Tensor) -> torch.Tensor:
    g = w.get(name)
    return y if g is None else y * g


def _lin(x, wt, b):
    y = x @ wt.t()
    return y if b is None else y + b


def block(w: W, p: str, x: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    """RMSNorm -> causal depthwise conv -> layer scale residual; RMSNorm -> Linear -> GELU -> Linear -> layer scale residual."""
    y = depthwise_conv(rms(x, w[f"{p}.norm.weight"], spec.eps), w[f"{p}.mixer.weight"], w.get(f"{p}.mixer.bias"))
    x = x + _scale(w, f"{p}.gamma", y)
    h = gelu(_lin(rms(x, w[f"{p}.ffn_norm.weight"], spec.eps), w[f"{p}.ffn.w1.weight"], w.get(f"{p}.ffn.w1.bias")))
    return x + _scale(w, f"{p}.ffn_gamma", _lin(h, w[f"{p}.ffn.w2.weight"], w.get(f"{p}.ffn.w2.bias")))


def enc_depths(spec: CodecSpec):
    return tuple(reversed(spec.dec_depths))


def enc_ratios(spec: CodecSpec):
    return tuple(reversed(spec.ratios))


# ---- the parts of smtts_test_codec_stage (what = 1 stem, 2 resampling into stage i, 4 the stage's blocks, 8 final norm + head)
def dec_stem(w: W, lat: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    return causal_conv(lat, w[f"{DEC}.stem.weight"], w.get(f"{DEC}.stem.bias"))


def dec_resample(w: W, i: int, x: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    return conv_transpose(x, w[f"{DEC}.up.{i}.weight"], w.get(f"{DEC}.up.{i}.bias"), spec.ratios[i - 1])


def dec_blocks(w: W, i: int, x: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    for j in range(spec.dec_depths[i]):
        x = block(w, f"{DEC}.stages.{i}.{j}", x, spec)
    return x


def dec_head(w: W, x: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    """-> (B, T, 1) audio"""
    if w.get(f"{DEC}.final_norm.weight") is not None:
        x = rms(x, w[f"{DEC}.final_norm.weight"], spec.eps)
    return causal_conv(x, w[f"{DEC}.head.weight"], w.get(f"{DEC}.head.bias"))


def enc_stem(w: W, audio: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    """audio (B, S) or (B, S, 1) -> (B, S, C0)"""
    if audio.dim() == 2:
        audio = audio[:, :, None]
    return causal_conv(audio, w[f"{ENC}.stem.weight"], w.get(f"{ENC}.stem.bias"))


def enc_resample(w: W, i: int, x: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    return causal_conv(x, w[f"{ENC}.down.{i}.weight"], w.get(f"{ENC}.down.{i}.bias"), stride=enc_ratios(spec)[i - 1])


def enc_blocks(w: W, i: int, x: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    for j in range(enc_depths(spec)[i]):
        x = block(w, f"{ENC}.stages.{i}.{j}", x, spec)
    return x


def enc_head(w: W, x: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    if w.get(f"{ENC}.final_norm.weight") is not None:
        x = rms(x, w[f"{ENC}.final_norm.weight"], spec.eps)
    return causal_conv(x, w[f"{ENC}.head.weight"], w.get(f"{ENC}.head.bias"))


def stage(w: W, part: str, i: int, what: int, x: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    """The fp64 statement of smtts_test_codec_stage(part, i, what) on x (B, T, C)."""
    dec = part == "decoder"
    if what & 1:
        x = (dec_stem if dec else enc_stem)(w, x, spec)
    if what & 2:
        x = (dec_resample if dec else enc_resample)(w, i, x, spec)
    if what & 4:
        x = (dec_blocks if dec else enc_blocks)(w, i, x, spec)
    if what & 8:
        x = (dec_head if dec else enc_head)(w, x, spec)
    return x


def decode(w: W, lat: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    """(B, T, latent) -> (B, 1, hop T), composed of the stages"""
    x = lat
    for i in range(spec.n_stages):
        x = stage(w, "decoder", i, (1 if i == 0 else 2) | 4 | (8 if i == spec.n_stages - 1 else 0), x, spec)
    return x.transpose(1, 2)


def encode(w: W, audio: torch.Tensor, spec: CodecSpec) -> torch.Tensor:
    """(B, 1, S) -> (B, S // hop, latent), composed of the stages"""
    x = audio[:, 0, : (audio.shape[-1] // spec.hop) * spec.hop]
    for i in range(spec.n_stages):
        x = stage(w, "encoder", i, (1 if i == 0 else 2) | 4 | (8 if i == spec.n_stages - 1 else 0), x, spec)
    return x
