"""Restatement the speaker-verifier tests hold the device to.

The network: SV(192) of the reference (models/sv/model.py) = speechbrain's ECAPA_TDNN(input_size=64, lin_neurons=192,
channels=[768,768,768,768,2304], kernel_sizes=[3,3,3,3,1], dilations=[1,2,3,5,1], attention_channels=192, res2net_scale=12,
se_channels=192, global_context=True) in eval mode.  speechbrain is not a dependency: the composition is restated here from recollection
(UNPINNED), every primitive is torch's own, and the module tree carries the state-dict names (speechbrain's wrappers nest
.conv.conv and .norm.norm) so that a state dict loads by name.  THE reference is `embed_rows`: every row alone at its own length (what
batch-1 inference computes).  `embed_batched` is speechbrain's batched form (squeeze-excite and pooling masked by the lengths, the
convolutions not: they reflect about the batch's end and read the padding): kept only to show the difference.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from smalltts_amd.weights import (SV_ATT, SV_CHANNELS, SV_DILATIONS, SV_DIM, SV_IN, SV_MFA, SV_MIN_FRAMES, SV_SCALE, SV_SE,
                                  sv_param_specs, synth_state_dict)

ASP_EPS = 1e-12


class _Conv(nn.Module):
    """Conv1d with "same" reflect padding of d (k - 1) / 2 frames each side"""
    def __init__(self, i, o, k, d=1):
        super().__init__()
        self.conv = nn.Conv1d(i, o, k, dilation=d)
        self.pad = d * (k - 1) // 2

    def forward(self, x):   # (B, C, T)
        if self.pad:
            x = F.pad(x, (self.pad, self.pad), mode="reflect")   # raises when pad >= T
        return self.conv(x)


class _Norm(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.norm = nn.BatchNorm1d(n)

    def forward(self, x):
        return self.norm(x)


class _TDNN(nn.Module):
    """conv, ReLU, BatchNorm, in that order"""
    def __init__(self, i, o, k, d):
        super().__init__()
        self.conv = _Conv(i, o, k, d)
        self.norm = _Norm(o)

    def forward(self, x):
        return self.norm(torch.relu(self.conv(x)))


class _Res2Net(nn.Module):
    def __init__(self, c, scale, d):
        super().__init__()
        self.scale = scale
        self.blocks = nn.ModuleList(_TDNN(c // scale, c // scale, 3, d) for _ in range(scale - 1))

    def forward(self, x):
        y = []
        for i, xi in enumerate(torch.chunk(x, self.scale, dim=1)):
            if i == 0:
                yi = xi
            elif i == 1:
                yi = self.blocks[0](xi)
            else:
                yi = self.blocks[i - 1](xi + yi)
            y.append(yi)
        return torch.cat(y, dim=1)


def _mask(lengths, T, dtype):
    """(B, 1, T) of ones in front of every row's length, or None"""
    if lengths is None:
        return None
    return (torch.arange(T)[None, :] < torch.as_tensor(lengths)[:, None]).to(dtype)[:, None, :]


class _SE(nn.Module):
    def __init__(self, c, se):
        super().__init__()
        self.conv1 = _Conv(c, se, 1)
        self.conv2 = _Conv(se, c, 1)

    def forward(self, x, lengths=None):
        m = _mask(lengths, x.shape[-1], x.dtype)
        s = x.mean(dim=2, keepdim=True) if m is None else (x * m).sum(dim=2, keepdim=True) / m.sum(dim=2, keepdim=True)
        return torch.sigmoid(self.conv2(torch.relu(self.conv1(s)))) * x


class _SERes2Net(nn.Module):
    def __init__(self, c, d):
        super().__init__()
        self.tdnn1 = _TDNN(c, c, 1, 1)
        self.res2net_block = _Res2Net(c, SV_SCALE, d)
        self.tdnn2 = _TDNN(c, c, 1, 1)
        self.se_block = _SE(c, SV_SE)

    def forward(self, x, lengths=None):
        return self.se_block(self.tdnn2(self.res2net_block(self.tdnn1(x))), lengths) + x


def _stats(x, w):
    """weighted mean and two-pass std over time; w sums to 1 over a row's frames"""
    mean = (w * x).sum(dim=2)
    std = torch.sqrt((w * (x - mean[:, :, None]) ** 2).sum(dim=2).clamp(min=ASP_EPS))
    return mean, std


class _ASP(nn.Module):
    def __init__(self, c, att):
        super().__init__()
        self.tdnn = _TDNN(3 * c, att, 1, 1)
        self.conv = _Conv(att, c, 1)

    def forward(self, x, lengths=None):
        T = x.shape[-1]
        m = _mask(lengths, T, x.dtype)
        if m is None:
            m = torch.ones(x.shape[0], 1, T, dtype=x.dtype)
        mean, std = _stats(x, m / m.sum(dim=2, keepdim=True))
        a = torch.cat([x, mean[:, :, None].expand(-1, -1, T), std[:, :, None].expand(-1, -1, T)], dim=1)
        a = self.conv(torch.tanh(self.tdnn(a)))
        a = torch.softmax(a.masked_fill(m == 0, float("-inf")), dim=2)
        mean, std = _stats(x, a)
        return torch.cat([mean, std], dim=1)[:, :, None]


class _ECAPA(nn.Module):
    def __init__(self):
        super().__init__()
        self.blocks = nn.ModuleList([_TDNN(SV_IN, SV_CHANNELS, 3, 1)] + [_SERes2Net(SV_CHANNELS, d) for d in SV_DILATIONS])
        self.mfa = _TDNN(SV_MFA, SV_MFA, 1, 1)
        self.asp = _ASP(SV_MFA, SV_ATT)
        self.asp_bn = _Norm(2 * SV_MFA)
        self.fc = _Conv(2 * SV_MFA, SV_DIM, 1)

    def forward(self, x, lengths=None):   # x (B, N, 64) -> (B, 192)
        x = self.blocks[0](x.transpose(1, 2))
        outs = []
        for blk in list(self.blocks)[1:]:
            x = blk(x, lengths)
            outs.append(x)
        x = self.mfa(torch.cat(outs, dim=1))
        return self.fc(self.asp_bn(self.asp(x, lengths)))[:, :, 0]


class SVRef(nn.Module):
    def __init__(self):
        super().__init__()
        self.ecapa = _ECAPA()

    def forward(self, x, lengths=None):
        return self.ecapa(x, lengths)


def state_dict(seed: int):
    """The synthetic verifier weights under the reference's own key names (no "sv." prefix), float32 torch tensors."""
    sd = synth_state_dict(sv_param_specs(), seed)
    return {k[len("sv."):]: torch.from_numpy(v.copy()) for k, v in sd.items()}


def build(seed: int, dtype=torch.float64) -> SVRef:
    m = SVRef()
    missing, unexpected = m.load_state_dict(state_dict(seed), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return m.to(dtype).eval()


@torch.no_grad()
def embed_rows(model: SVRef, x: torch.Tensor, lengths) -> torch.Tensor:
    """THE reference: every row alone at its own length; a row under 6 frames has no embedding and stays 0.0."""
    dt = next(model.parameters()).dtype
    out = torch.zeros(x.shape[0], SV_DIM, dtype=dt)
    for b, n in enumerate(int(v) for v in lengths):
        if n >= SV_MIN_FRAMES:
            out[b] = model(x[b:b + 1, :n].to(dt))[0]
    return out


@torch.no_grad()
def embed_batched(model: SVRef, x: torch.Tensor, lengths) -> torch.Tensor:
    dt = next(model.parameters()).dtype
    return model(x.to(dt), [int(v) for v in lengths])


def cosine(emb, ref, K: int = 1) -> np.ndarray:
    """float64 cosine of row b of emb against row b // K of ref, F.cosine_similarity's rule (each norm clamped at 1e-8)."""
    a = np.asarray(emb, dtype=np.float64)
    r = np.repeat(np.asarray(ref, dtype=np.float64), K, axis=0)
    na = np.maximum(np.sqrt((a * a).sum(axis=1)), 1e-8)
    nr = np.maximum(np.sqrt((r * r).sum(axis=1)), 1e-8)
    return (a * r).sum(axis=1) / (na * nr)
