"""Restatements the recogniser and CTC tests hold the device to.

The network: ASR(64) of the reference (models/asr.py) = depthwise ConvTranspose x4, torchaudio's Conformer (7 layers, width 64, 16 heads,
FFN 1024, depthwise kernel 9), Linear 64 -> 198, log-softmax.  torchaudio is not a dependency: the composition is restated here from
recollection (UNPINNED), every primitive is torch's own module, and the module tree carries the reference's state-dict names
so that a state dict loads by name.  THE reference is `logprobs_rows`: every row alone at its own length (what batch-1 inference
computes).  `logprobs_batched` is torchaudio's batched form (keys masked, the conv module not): kept only to show the difference.

CTC: `ctc_nll` is the forward recursion in numpy float64, `greedy` the argmax / collapse / drop-blank transcript.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from smalltts_amd.weights import (ASR_CONV_K, ASR_DIM, ASR_FF, ASR_HEADS, ASR_LAYERS, ASR_UPSAMPLE, PHONEME_VOCAB, asr_param_specs,
                                  synth_state_dict)


class _FFN(nn.Module):
    def __init__(self, d, ff):
        super().__init__()
        self.sequential = nn.Sequential(nn.LayerNorm(d), nn.Linear(d, ff), nn.SiLU(), nn.Dropout(0.0), nn.Linear(ff, d), nn.Dropout(0.0))

    def forward(self, x):
        return self.sequential(x)


class _Conv(nn.Module):
    def __init__(self, d, k):
        super().__init__()
        self.layer_norm = nn.LayerNorm(d)
        self.sequential = nn.Sequential(nn.Conv1d(d, 2 * d, 1), nn.GLU(dim=1), nn.Conv1d(d, d, k, padding=(k - 1) // 2, groups=d),
                                        nn.BatchNorm1d(d), nn.SiLU(), nn.Conv1d(d, d, 1), nn.Dropout(0.0))

    def forward(self, x):   # (B, T, D)
        return self.sequential(self.layer_norm(x).transpose(1, 2)).transpose(1, 2)


class _Layer(nn.Module):
    def __init__(self, d, ff, heads, k):
        super().__init__()
        self.ffn1 = _FFN(d, ff)
        self.self_attn_layer_norm = nn.LayerNorm(d)
        self.self_attn = nn.MultiheadAttention(d, heads, dropout=0.0, batch_first=True)
        self.conv_module = _Conv(d, k)
        self.ffn2 = _FFN(d, ff)
        self.final_layer_norm = nn.LayerNorm(d)

    def forward(self, x, key_padding_mask):
        x = self.ffn1(x) * 0.5 + x
        y = self.self_attn_layer_norm(x)
        y, _ = self.self_attn(y, y, y, key_padding_mask=key_padding_mask, need_weights=False)
        x = y + x
        x = self.conv_module(x) + x
        x = self.ffn2(x) * 0.5 + x
        return self.final_layer_norm(x)


class _Encoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.conformer_layers = nn.ModuleList(_Layer(ASR_DIM, ASR_FF, ASR_HEADS, ASR_CONV_K) for _ in range(ASR_LAYERS))


class _Upsample(nn.Module):
    def __init__(self):
        super().__init__()
        self.deconv = nn.ConvTranspose1d(ASR_DIM, ASR_DIM, ASR_UPSAMPLE, stride=ASR_UPSAMPLE, groups=ASR_DIM)


class ASRRef(nn.Module):
    def __init__(self):
        super().__init__()
        self.upsample = _Upsample()
        self.encoder = _Encoder()
        self.proj = nn.Linear(ASR_DIM, PHONEME_VOCAB)

    def forward(self, x, lengths=None):
        """x (B, N, 64), lengths (B) latent frames or None -> log-probs (B, 4 N, 198).  With lengths: torchaudio's batched form."""
        y = self.upsample.deconv(x.transpose(1, 2)).transpose(1, 2)
        kpm = None
        if lengths is not None:
            t = torch.arange(y.shape[1])[None, :]
            kpm = t >= (ASR_UPSAMPLE * torch.as_tensor(lengths))[:, None]
        for layer in self.encoder.conformer_layers:
            y = layer(y, kpm)
        return torch.log_softmax(self.proj(y), dim=-1)


def state_dict(seed: int):
    """The synthetic recogniser weights under the reference's own key names (no "asr." prefix), float32 torch tensors."""
    sd = synth_state_dict(asr_param_specs(), seed)
    return {k[len("asr."):]: torch.from_numpy(v.copy()) for k, v in sd.items()}


def build(seed: int, dtype=torch.float64) -> ASRRef:
    m = ASRRef()
    missing, unexpected = m.load_state_dict(state_dict(seed), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


@torch.no_grad()
def logprobs_rows(model: ASRRef, x: torch.Tensor, lengths) -> torch.Tensor:
    """THE reference: every row alone at its own length; frames at and behind 4 n_b are 0.0."""
    dt = next(model.parameters()).dtype
    B, N, _ = x.shape
    out = torch.zeros(B, ASR_UPSAMPLE * N, PHONEME_VOCAB, dtype=dt)
    for b, n in enumerate(int(v) for v in lengths):
        if n > 0:
            out[b, :ASR_UPSAMPLE * n] = model(x[b:b + 1, :n].to(dt))[0]
    return out


@torch.no_grad()
def logprobs_batched(model: ASRRef, x: torch.Tensor, lengths) -> torch.Tensor:
    dt = next(model.parameters()).dtype
    return model(x.to(dt), [int(v) for v in lengths])


def _lse(rows: np.ndarray) -> np.ndarray:
    """log-sum-exp over axis 0, maximum first; -inf (not NaN) where every operand is -inf"""
    m = rows.max(axis=0)
    mm = np.where(np.isneginf(m), 0.0, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(np.isneginf(m), -np.inf, mm + np.log(np.exp(rows - mm).sum(axis=0)))


def ctc_nll(logp: np.ndarray, t_len: int, target) -> float:
    """-log p(target | logp[:t_len]) under CTC with blank 0, float64; +inf for an empty or infeasible row."""
    lp = np.asarray(logp, dtype=np.float64)
    tgt = [int(v) for v in target]
    L = len(tgt)
    if t_len <= 0 or L <= 0:
        return np.inf
    ext = np.zeros(2 * L + 1, dtype=np.int64)
    ext[1::2] = tgt
    S = len(ext)
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
    ninf = np.full(2, -np.inf)
    alpha = np.full(S, -np.inf)
    alpha[0] = lp[0, 0]
    alpha[1] = lp[0, ext[1]]
    for t in range(1, t_len):
        a1 = np.concatenate([ninf[:1], alpha[:-1]])
        a2 = np.where(skip, np.concatenate([ninf, alpha[:-2]]), -np.inf)
        alpha = _lse(np.stack([alpha, a1, a2])) + lp[t, ext]
    return float(-_lse(np.stack([alpha[S - 1:S], alpha[S - 2:S - 1]]))[0])


def greedy(logp: np.ndarray, t_len: int):
    """Per-frame argmax (lowest class on ties), runs collapsed, blanks dropped."""
    am = np.argmax(np.asarray(logp)[:t_len], axis=-1) if t_len > 0 else np.zeros(0, dtype=np.int64)
    return [int(c) for i, c in enumerate(am) if c != 0 and (i == 0 or c != am[i - 1])]


def clamp_window(p0: int, p1: int, P: int):
    p0 = min(max(int(p0), 0), P)
    p1 = min(max(int(p1), 0), P)
    return p0, p1
