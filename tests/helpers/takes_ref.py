"""Numpy restatements for the takes tests (test infrastructure, not product code): the definitions of include/smalltts_hip.h
smtts_take_scores / smtts_take_select written out once more, and text-mass buffers with planted defects.

* take_scores_ref: the four integer features and the float32 total of every row, one single-precision operation per step;
* take_select_ref: the winner of every group and the gathered rows, by numpy indexing;
* planted: a clean monotone mass and its "skip", "stall" and "idle" variants.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

F32 = np.float32
SHAPES = [(40, 15, 0), (33, 15, 3), (12, 5, 0), (225, 198, 0)]   # (N, P, p0) of the planted cases
VARIANTS = ("clean", "skip", "stall", "idle")


def take_scores_ref(mass, spans, path_score, ns, p0, p1, weights=(1.0, 2.0, 1.0, 1.0), tau_token=0.1,
                    tau_frame=0.1) -> Tuple[np.ndarray, np.ndarray]:
    """mass (B, N, P) fp32, spans (B, P, 2) int32, path_score (B) fp32, ns / p0 / p1 B integers -> (feat int32 (B, 4) = (cells, skipped,
    longest, idle), total fp32 (B))."""
    mass = np.asarray(mass, F32)
    spans = np.asarray(spans, np.int32)
    path_score = np.asarray(path_score, F32)
    B, N, P = mass.shape
    w = [F32(v) for v in weights]
    tt, tf = F32(tau_token), F32(tau_frame)
    feat = np.zeros((B, 4), np.int32)
    total = np.full((B,), np.inf, F32)
    for b in range(B):
        n = max(0, min(int(ns[b]), N)); a = max(0, min(int(p0[b]), P)); e = max(0, min(int(p1[b]), P))
        Pw = e - a
        if n <= 0 or Pw <= 0:
            continue
        cells = skipped = longest = idle = 0
        for p in range(a, e):
            first, last = int(spans[b, p, 0]), int(spans[b, p, 1])
            if first < 0 or last < first:
                skipped += 1
                continue
            first, last = min(first, n - 1), min(last, n - 1)
            length = last - first + 1
            cells += length
            longest = max(longest, length)
            if not bool(np.any(mass[b, first:last + 1, p] >= tt)):   # (a NaN satisfies no comparison)
                skipped += 1
        for f in range(n):
            if not bool(np.any(mass[b, f, a:e] >= tf)):
                idle += 1
        feat[b] = (cells, skipped, longest, idle)
        with np.errstate(divide="ignore", invalid="ignore"):
            c0 = F32(path_score[b] / F32(cells))
            c1 = F32(F32(skipped) / F32(Pw))
            c2 = F32(F32(longest) / F32(n))
            c3 = F32(F32(idle) / F32(n))
            t = F32(F32(w[0] * c0) + F32(w[1] * c1))
            t = F32(t + F32(w[2] * c2))
            total[b] = F32(t + F32(w[3] * c3))
    return feat, total


def winners_ref(total, K: int) -> np.ndarray:
    """total (G * K) fp32, piece-major -> winner (G) int32: the lowest k with the smallest key, key = NaN ? +inf : total."""
    t = np.asarray(total, F32).reshape(-1, K)
    out = np.zeros((t.shape[0],), np.int32)
    for g in range(t.shape[0]):
        best, win = (F32(np.inf) if np.isnan(t[g, 0]) else t[g, 0]), 0
        for k in range(1, K):
            s = F32(np.inf) if np.isnan(t[g, k]) else t[g, k]
            if s < best:
                best, win = s, k
        out[g] = win
    return out


def take_select_ref(total, K: int, x, ns, spans=None, mass=None):
    """-> (x_win, n_win, spans_win or None, mass_win or None, winner), the winners' rows by numpy indexing."""
    win = winners_ref(total, K)
    rows = np.arange(win.shape[0]) * K + win
    pick = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a)[rows])
    return pick(x), np.asarray(ns, np.int32)[rows], pick(spans), pick(mass), win


def planted(N: int, P: int, p0: int, variant: str = "clean", lo: float = 0.002, hi: float = 0.8) -> np.ndarray:
    """A text-mass buffer (N, P) fp32: `lo` everywhere, `hi` on a monotone map pi of the frames onto the tokens [p0, P).
    clean: pi(f) = p0 + f * Pw // N.  skip: token p0 + 2's frames are given to its successor.  stall: from frame N // 3 on one token
    holds until the remaining tokens are crammed into the last frames, one frame each.  idle: N // 5 frames from N // 2 on carry no
    text mass at all."""
    assert variant in VARIANTS and 0 <= p0 < P and N >= 1
    Pw = P - p0
    pi = [p0 + f * Pw // N for f in range(N)]
    if variant == "skip":
        pi = [p + 1 if p == p0 + 2 else p for p in pi]
    elif variant == "stall":
        f0 = N // 3
        held = pi[f0]
        rest = P - 1 - held                      # tokens still to come behind the held one
        for f in range(f0, N):
            pi[f] = held if f < N - rest else held + (f - (N - rest)) + 1
    m = np.full((N, P), lo, F32)
    for f, p in enumerate(pi):
        m[f, p] = F32(hi)
    if variant == "idle":
        f0 = N // 2
        m[f0: f0 + N // 5, :] = F32(0.0)
    return m
