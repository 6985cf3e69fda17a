"""Numpy restatements for the repair tests (test infrastructure, not product code): the definitions of include/smalltts_hip.h
smtts_repair_plan / smtts_repair_keep written out once more from the header's text.

* repair_plan_ref: the pin mask and (bad tokens, freed frames) of every row;
* repair_keep_ref: which rows the repaired take replaces, and the merged buffers (copies: the inputs are left alone).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

F32 = np.float32


def repair_plan_ref(mass, spans, ns, p0, p1, keep=None, tau_token=0.1, max_span=8, margin=2) -> Tuple[np.ndarray, np.ndarray]:
    """mass (B, N, P) fp32, spans (B, P, 2) int32, ns / p0 / p1 B integers, keep (B, N) or None -> (pin uint8 (B, N), counts int32
    (B, 2) = (bad tokens, frames below n with pin 0))."""
    mass = np.asarray(mass, F32)
    spans = np.asarray(spans, np.int32)
    B, N, P = mass.shape
    tt = F32(tau_token)
    pin = np.zeros((B, N), np.uint8)
    counts = np.zeros((B, 2), np.int32)
    for b in range(B):
        n = max(0, min(int(ns[b]), N)); a = max(0, min(int(p0[b]), P)); e = max(0, min(int(p1[b]), P))
        if n <= 0 or e <= a:
            continue
        freed = np.zeros(n, bool)
        bad = 0
        for p in range(a, e):
            first, last = int(spans[b, p, 0]), int(spans[b, p, 1])
            if first < 0 or last < first:
                bad += 1                                             # an empty span: bad, frees nothing
                continue
            first, last = min(first, n - 1), min(last, n - 1)
            if last - first + 1 > int(max_span) or not bool(np.any(mass[b, first:last + 1, p] >= tt)):   # (a NaN satisfies no comparison)
                bad += 1
                freed[max(0, first - int(margin)): min(n - 1, last + int(margin)) + 1] = True
        row = ~freed
        if keep is not None:
            row |= np.asarray(keep)[b, :n] != 0
        pin[b, :n] = row
        counts[b] = (bad, int(n - row.sum()))
    return pin, counts


def replace_ref(total_cur, total_new, counts) -> np.ndarray:
    """-> replace (G) bool: counts[g][1] > 0 and key(total_new[g]) < key(total_cur[g]), key = NaN ? +inf : total."""
    key = lambda t: np.where(np.isnan(t), F32(np.inf), t).astype(F32)
    return (np.asarray(counts)[:, 1] > 0) & (key(np.asarray(total_new, F32)) < key(np.asarray(total_cur, F32)))


def repair_keep_ref(total_cur, total_new, counts, feat_cur, feat_new, x_cur, x_new, spans_cur=None, spans_new=None, mass_cur=None,
                    mass_new=None):
    """-> (total_out, feat_out, kept int32, x, spans or None, mass or None): the merged buffers."""
    rep = replace_ref(total_cur, total_new, counts)

    def merge(cur, new):
        if cur is None:
            return None
        out = np.array(cur, copy=True)
        out[rep] = np.asarray(new)[rep]
        return out
    return (merge(np.asarray(total_cur, F32), total_new), merge(np.asarray(feat_cur, np.int32), feat_new), rep.astype(np.int32),
            merge(x_cur, x_new), merge(spans_cur, spans_new), merge(mass_cur, mass_new))
