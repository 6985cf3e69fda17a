"""The definition of smtts_ctc_align (include/smalltts_hip.h) restated in numpy float32, one operation at a time, and the
brute force that holds the restatement: every valid CTC path of a tiny row enumerated in float64.

align() takes three switches that each break one rule of the definition; tests/test_ctc_align_cpu.py shows that every broken version
fails the brute force on at least one case, i.e. that the cases can tell."""
import itertools

import numpy as np

F32 = np.float32
NEG = F32(-np.inf)


def clamp(v, lo, hi):
    v = int(v)
    return lo if v < lo else hi if v > hi else v


def labels_of(tokens, p0, p1, C):
    """The extended labels [blank, l_0, blank, ..., blank] of tokens[p0 : p1), every token clamped into [1, C)."""
    lab = [0]
    for t in tokens[p0:p1]:
        lab += [clamp(t, 1, C - 1), 0]
    return np.asarray(lab, np.int64)


def align(logp, t_len, tokens, p0, p1, *, ties="stay", skip_equal=False, end="both"):
    """One row.  logp (T, C) float32, tokens (P,) -> dict(spans (P, 2) i32, tok_logp (P,) f32, frame_tok (T,) i32, score f32,
    state (list of t_len states, or None when the row is not aligned)).  ties "move", skip_equal True and end "last" are the WRONG
    versions: ties prefer the larger move, the skip crosses equal labels, the path may only end in the last blank."""
    lp = np.asarray(logp, F32)
    T, C = lp.shape
    tokens = [int(t) for t in np.asarray(tokens).reshape(-1)]
    P = len(tokens)
    tb, p0, p1 = clamp(t_len, 0, T), clamp(p0, 0, P), clamp(p1, 0, P)
    L = p1 - p0
    out = dict(spans=np.full((P, 2), -1, np.int32), tok_logp=np.zeros(P, F32), frame_tok=np.full(T, -1, np.int32), score=NEG, state=None)
    if tb == 0 or L <= 0:
        return out
    lab = labels_of(tokens, p0, p1, C)
    S = 2 * L + 1
    idx = np.arange(S)
    skip = np.zeros(S, bool)
    for s in range(3, S, 2):
        skip[s] = skip_equal or lab[s] != lab[s - 2]
    gt = (lambda a, v: a > v) if ties == "stay" else (lambda a, v: a >= v)
    delta = np.full(S, NEG, F32)
    delta[0], delta[1] = lp[0, 0], lp[0, lab[1]]
    moves = np.zeros((tb, S), np.int64)
    with np.errstate(invalid="ignore"):
        for t in range(1, tb):
            prev = delta
            v = prev.copy()
            m = np.zeros(S, np.int64)
            a1 = np.concatenate(([NEG], prev[:-1]))
            c1 = (idx >= 1) & gt(a1, v)
            v, m = np.where(c1, a1, v), np.where(c1, 1, m)
            a2 = np.concatenate(([NEG, NEG], prev[:-2]))
            c2 = skip & gt(a2, v)
            v, m = np.where(c2, a2, v), np.where(c2, 2, m)
            delta = (v + lp[t, lab]).astype(F32)
            moves[t] = m
        e = S - 1 if end == "last" else (S - 2 if delta[S - 2] > delta[S - 1] else S - 1)
    out["score"] = F32(delta[e])
    if not out["score"] > NEG:                                 # -inf and NaN: not aligned
        return out
    state = [0] * tb
    s = e
    for t in range(tb - 1, 0, -1):
        state[t] = s
        s = max(s - int(moves[t, s]), 0)
    state[0] = s
    out["state"] = state
    for p in range(p0, p1):
        fr = [t for t in range(tb) if state[t] == 2 * (p - p0) + 1]
        if fr:
            out["spans"][p] = (fr[0], fr[-1])
            acc = F32(0.0)
            with np.errstate(invalid="ignore"):
                for t in fr:
                    acc = F32(acc + lp[t, clamp(tokens[p], 1, C - 1)])
            out["tok_logp"][p] = acc
    for t in range(tb):
        if state[t] & 1:
            out["frame_tok"][t] = p0 + (state[t] >> 1)
    return out


def align_batch(logp, t_len, tokens, p0, p1):
    """(B, T, C), (B,), (B, P), (B,), (B,) -> spans (B, P, 2), tok_logp (B, P), frame_tok (B, T), score (B,)."""
    rows = [align(logp[b], t_len[b], tokens[b], p0[b], p1[b]) for b in range(len(t_len))]
    return (np.stack([r["spans"] for r in rows]), np.stack([r["tok_logp"] for r in rows]), np.stack([r["frame_tok"] for r in rows]),
            np.asarray([r["score"] for r in rows], F32))


def brute_force(logp, tokens):
    """Every valid path of the whole row in float64 -> (score, state list) of the best one, (-inf, None) when there is none.  Among
    paths of equal score (exact sums: quantised inputs) the definition's choice is the one whose states are largest read from the
    last frame backwards: the end prefers S - 1, every step prefers staying, then one step."""
    lp = np.asarray(logp, np.float64)
    T, C = lp.shape
    lab = labels_of([int(t) for t in tokens], 0, len(tokens), C)
    S = len(lab)
    def paths(prefix):
        if len(prefix) == T:
            if prefix[-1] >= S - 2:
                yield tuple(prefix)
            return
        a = prefix[-1]
        for b in (a, a + 1, a + 2):
            if b < S and (b - a < 2 or (b & 1 and lab[b] != lab[a])):
                yield from paths(prefix + [b])

    best = (-np.inf, None)
    for path in itertools.chain(paths([0]), paths([1])):
        sc = 0.0
        for t, s in enumerate(path):
            sc += lp[t, lab[s]]
        if not sc > -np.inf:
            continue
        if best[1] is None or (sc, path[::-1]) > (best[0], tuple(best[1][::-1])):
            best = (sc, list(path))
    return best
