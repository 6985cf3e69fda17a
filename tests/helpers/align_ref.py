"""Numpy / torch restatements for the word-timing tests (test infrastructure, not product code).

* dp_align: the float32 recurrence of smtts_align_path, one single-precision operation per step, the same tie rule;
* brute_force_paths: every monotone path of a small grid (what dp_align is held to on the CPU);
* text_mass_fp64: the text-attention tap of one attention call on raw projections, in fp64 (the fp64 restatement of
  tests/test_kernels_gpu.py's attention with the probabilities read out instead of multiplied into V);
* sampler_text_mass: the tap inside the DMD sampler, composed from the oracle/dit_stages.py pieces.
"""
from __future__ import annotations

import itertools
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

F32 = np.float32


def dp_align(mass: np.ndarray, n: int, p0: int, p1: int) -> Tuple[np.ndarray, float, List[Tuple[int, int]]]:
    """mass (N, P) float32 -> (spans int32 (P, 2), score float32, path [(frame, token), ...] from the start).
    c = 1 - mass (fp32); D[n][p] = c + min(D[n-1][p-1], D[n-1][p], D[n][p-1]) (fp32); ties: diagonal, then (n-1, p), then (n, p-1)."""
    mass = np.asarray(mass, F32)
    N, P = mass.shape
    n = max(0, min(int(n), N)); p0 = max(0, min(int(p0), P)); p1 = max(0, min(int(p1), P))
    spans = np.full((P, 2), -1, np.int32)
    Pw = p1 - p0
    if n <= 0 or Pw <= 0:
        return spans, F32(0.0), []
    c = (F32(1.0) - mass[:n, p0:p1]).astype(F32)
    D = np.full((n, Pw), np.inf, F32)
    bp = np.zeros((n, Pw), np.uint8)
    for i in range(n):
        for j in range(Pw):
            if i == 0 and j == 0:
                D[0, 0] = c[0, 0]
                continue
            diag = D[i - 1, j - 1] if i > 0 and j > 0 else F32(np.inf)
            up = D[i - 1, j] if i > 0 else F32(np.inf)
            left = D[i, j - 1] if j > 0 else F32(np.inf)
            best, k = diag, 0
            if up < best:
                best, k = up, 1
            if left < best:
                best, k = left, 2
            D[i, j] = F32(c[i, j] + best)
            bp[i, j] = k
    i, j = n - 1, Pw - 1
    path = [(i, j)]
    while i > 0 or j > 0:
        k = 2 if i == 0 else 1 if j == 0 else int(bp[i, j])
        if k == 0:
            i, j = i - 1, j - 1
        elif k == 1:
            i -= 1
        else:
            j -= 1
        path.append((i, j))
    path.reverse()
    for (i, j) in path:
        t = p0 + j
        if spans[t, 0] < 0:
            spans[t, 0] = i
        spans[t, 1] = i
    return spans, D[n - 1, Pw - 1], [(i, p0 + j) for i, j in path]


def brute_force_paths(cost: np.ndarray):
    """Every monotone path (0,0) -> (N-1,P-1) with steps (1,1), (1,0), (0,1) of a small cost grid: -> [(float64 cost, path), ...]."""
    N, P = cost.shape
    out = []

    def walk(i, j, acc, path):
        acc = acc + float(cost[i, j])
        path = path + [(i, j)]
        if i == N - 1 and j == P - 1:
            out.append((acc, path))
            return
        if i + 1 < N and j + 1 < P:
            walk(i + 1, j + 1, acc, path)
        if i + 1 < N:
            walk(i + 1, j, acc, path)
        if j + 1 < P:
            walk(i, j + 1, acc, path)

    walk(0, 0, 0.0, [])
    return out


def spans_of_path(path: Iterable[Tuple[int, int]], P: int) -> np.ndarray:
    spans = np.full((P, 2), -1, np.int32)
    for i, t in path:
        if spans[t, 0] < 0:
            spans[t, 0] = i
        spans[t, 1] = i
    return spans


def path_score_f64(mass: np.ndarray, path: Iterable[Tuple[int, int]]) -> float:
    """the cost of a path with the kernel's fp32 costs summed in float64"""
    m = np.asarray(mass, F32)
    return float(sum(np.float64(F32(1.0) - m[i, t]) for i, t in path))


def text_mass_fp64(qkvg, qw, kw, eps, rope, rot, H, dh, kr, kt, ms, mr, mt) -> torch.Tensor:
    """fp64 restatement of dit.py:95-119 up to the softmax on raw projections (B, N, 4 H dh): -> (B, N, P), the mean over heads of
    each frame's probability on each text key; zero for frames / text keys the masks exclude and for rows without a key."""
    B, N, _ = qkvg.shape
    D = H * dh
    x = qkvg.double()
    q, k = (x[..., i * D:(i + 1) * D].reshape(B, N, H, dh) for i in range(2))
    rms = lambda t, w: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    q, k = rms(q, qw), rms(k, kw)

    def rot_pairs(t):
        a = rope.double()[:N, :rot][None, :, None, 0::2]
        te, to = t[..., 0:rot:2], t[..., 1:rot:2]
        out = t.clone()
        out[..., 0:rot:2] = te * a.cos() - to * a.sin()
        out[..., 1:rot:2] = to * a.cos() + te * a.sin()
        return out
    q, k = rot_pairs(q).transpose(1, 2), rot_pairs(k).transpose(1, 2)
    ms = ms if ms is not None else torch.ones(B, N, dtype=torch.bool)
    keys, masks = [k], [ms]
    if kr is not None:
        keys.append(kr.double())
        masks.append(mr if mr is not None else torch.ones(B, kr.shape[2], dtype=torch.bool))
    P = kt.shape[2]
    keys.append(kt.double())
    masks.append(mt if mt is not None else torch.ones(B, P, dtype=torch.bool))
    K, Mk = torch.cat(keys, 2), torch.cat(masks, 1)
    s = q @ K.transpose(-1, -2) / dh ** 0.5
    s = s.masked_fill(~Mk[:, None, None, :], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    return p[..., -P:].mean(1) * ms.double()[..., None]


def block_text_probs(w, l: int, x, mask, rows, cache) -> torch.Tensor:
    """The joint attention of DiT block l on the residual x, from the oracle/dit_stages.py pieces, with one-hot values on the text
    keys: the masked softmax's output IS the probability of each text key.  -> (B, H, N, P) fp64."""
    from oracle import dit_stages as S
    B, N, _ = x.shape
    p = f"dit.transformer_blocks.{l}"
    sh_a, sc_a = S.block_mod(rows, l)[:2]
    y = S.adaln(x, sh_a, sc_a)
    q = S._lin(w, f"{p}.attn.to_q", y).reshape(B, N, S.HEADS, S.DH)
    k = S._lin(w, f"{p}.attn.to_k_self", y).reshape(B, N, S.HEADS, S.DH)
    q = S.rms_norm(q, S._d(w, f"{p}.attn.q_norm.weight"), 1e-6)
    k = S.rms_norm(k, S._d(w, f"{p}.attn.k_norm.weight"), 1e-6)
    a = S.rope_half_angles(N, S.ROPE_DIM)
    rot = lambda z: torch.cat([S.rotate_pairs(z[..., :S.ROPE_DIM], a[None, :, None, :]), z[..., S.ROPE_DIM:]], -1)
    q, k = rot(q), rot(k)
    kk, km = [k.transpose(1, 2)], [mask]
    if cache.get("k_ref") is not None and cache["k_ref"].shape[3] > 0:
        kk.append(cache["k_ref"][l].to(torch.float64))
        km.append(cache["ref_mask"])
    kk.append(cache["k_text"][l].to(torch.float64))
    km.append(cache["ph_mask"])
    K = torch.cat(kk, 2)
    P = cache["k_text"].shape[3]
    V = torch.zeros(B, S.HEADS, K.shape[2], P, dtype=torch.float64)
    V[:, :, K.shape[2] - P:, :] = torch.eye(P, dtype=torch.float64)
    return S.attention(q.transpose(1, 2), K, V, torch.cat(km, 1), 1.0 / S.DH ** 0.5)


def sampler_text_mass(w, cache, ph_mask, mask, noise, num_steps: int, steps: Optional[Sequence[int]] = None,
                      layers: Optional[Sequence[int]] = None, heads: Optional[Sequence[int]] = None):
    """The DMD sampler (oracle/dit_oracle.py sample_dmd) in fp64, stage by stage, with the tap: -> (x (B,N,64), mass (B,N,P)), mass
    the mean over the selected (step, layer, head) triples (defaults: last step, all layers, all heads), zero outside `mask`."""
    from oracle import dit_oracle as O
    from oracle import dit_stages as S
    B, N = mask.shape
    steps = [num_steps - 1] if steps is None else [int(s) % num_steps for s in steps]
    layers = list(range(S.NBLK)) if layers is None else [int(v) for v in layers]
    heads = list(range(S.HEADS)) if heads is None else [int(v) for v in heads]
    c = dict(cache, ph_mask=ph_mask)
    P = c["k_text"].shape[3]
    mass = torch.zeros(B, N, P, dtype=torch.float64)
    x = torch.zeros(B, N, 64, dtype=torch.float64)
    ts = np.linspace(1, 0, num_steps, dtype=np.float32)
    for i, tv in enumerate(ts):
        a, s = O.alpha_sigma(float(tv))
        x_t = float(a) * x + float(s) * noise[i].to(torch.float64)
        rows = S.mod_table(w, torch.full((B,), float(tv)))
        h = S.embed(w, x_t, mask)
        for l in range(S.NBLK):
            if i in steps and l in layers:
                mass += block_text_probs(w, l, h, mask, rows, c)[:, heads].sum(1)
            h = S.dit_block(w, l, h, mask, rows, c)
        v = S.head(w, S.next_image(h, rows, S.NBLK))
        x = float(a) * x_t - float(s) * v
    mass = mass / (len(set(steps)) * len(set(layers)) * len(set(heads))) * mask.to(torch.float64)[..., None]
    return x, mass
