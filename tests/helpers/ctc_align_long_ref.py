"""The definition of smtts_ctc_align (include/smalltts_hip.h), which smtts_ctc_align_long shares, restated in numpy
float32 with a vectorised tail: tests/helpers/ctc_align_ref.align walks every (token, frame) pair in Python behind the trace, which is
too slow past a few thousand frames.  Here the forward pass works in preallocated arrays, the trace is one Python loop over the frames,
and spans, tok_logp and frame_tok come from array operations: tok_logp adds the k-th frame of every token's span in one step, k
ascending, so that every token's sum is still a chain of single fp32 adds with t ascending.  tests/test_ctc_align_long_cpu.py holds
this file to ctc_align_ref.align bit for bit, states included."""
import numpy as np

F32 = np.float32
NEG = F32(-np.inf)


def clamp(v, lo, hi):
    v = int(v)
    return lo if v < lo else hi if v > hi else v


def align(logp, t_len, tokens, p0, p1):
    """One row.  logp (T, C) float32, tokens (P,) -> dict(spans (P, 2) i32, tok_logp (P,) f32, frame_tok (T,) i32, score f32, state
    (int array of t_len states, or None when the row is not aligned))."""
    lp = np.asarray(logp, F32)
    T, C = lp.shape
    tok = np.clip(np.asarray(tokens, np.int64).reshape(-1), 1, C - 1)
    P = tok.shape[0]
    tb, p0, p1 = clamp(t_len, 0, T), clamp(p0, 0, P), clamp(p1, 0, P)
    L = p1 - p0
    out = dict(spans=np.full((P, 2), -1, np.int32), tok_logp=np.zeros(P, F32), frame_tok=np.full(T, -1, np.int32), score=NEG, state=None)
    if tb == 0 or L <= 0:
        return out
    S = 2 * L + 1
    lab = np.zeros(S, np.int64)
    lab[1::2] = tok[p0:p1]
    skip = np.zeros(S, bool)
    skip[3::2] = lab[3::2] != lab[1:-2:2]
    delta = np.full(S, NEG, F32)
    delta[0], delta[1] = lp[0, 0], lp[0, lab[1]]
    moves = np.zeros((tb, S), np.int8)
    a1, a2 = np.full(S, NEG, F32), np.full(S, NEG, F32)
    with np.errstate(invalid="ignore"):
        for t in range(1, tb):
            a1[1:], a2[2:] = delta[:-1], delta[:-2]
            v = delta.copy()
            c1 = a1 > v                                        # (a1[0] = -inf is never greater: s >= 1)
            v[c1] = a1[c1]
            c2 = skip & (a2 > v)
            v[c2] = a2[c2]
            m = moves[t]
            m[c1], m[c2] = 1, 2
            delta = v + lp[t, lab]
        e = S - 2 if delta[S - 2] > delta[S - 1] else S - 1
    out["score"] = F32(delta[e])
    if not out["score"] > NEG:                                 # -inf and NaN: not aligned
        return out
    state = np.zeros(tb, np.int64)
    s = e
    for t in range(tb - 1, 0, -1):
        state[t] = s
        s = max(s - int(moves[t, s]), 0)
    state[0] = s
    out["state"] = state
    on = np.flatnonzero(state & 1)                             # the label frames, t ascending
    j = state[on] >> 1
    first, last = np.full(L, -1, np.int64), np.full(L, -1, np.int64)
    first[j[::-1]] = on[::-1]                                  # repeated indices: the last assignment stays, i.e. the smallest t
    last[j] = on
    out["spans"][p0:p1, 0], out["spans"][p0:p1, 1] = first, last
    out["frame_tok"][on] = p0 + j
    have = first >= 0
    n = np.where(have, last - first + 1, 0)
    acc = np.zeros(L, F32)
    cls = tok[p0:p1]
    with np.errstate(invalid="ignore"):
        for k in range(int(n.max()) if L else 0):
            w = np.flatnonzero(n > k)
            acc[w] = acc[w] + lp[first[w] + k, cls[w]]
    out["tok_logp"][p0:p1] = acc
    return out


def align_batch(logp, t_len, tokens, p0, p1):
    """(B, T, C), (B,), (B, P), (B,), (B,) -> spans (B, P, 2), tok_logp (B, P), frame_tok (B, T), score (B,)."""
    rows = [align(logp[b], t_len[b], tokens[b], p0[b], p1[b]) for b in range(len(t_len))]
    return (np.stack([r["spans"] for r in rows]), np.stack([r["tok_logp"] for r in rows]), np.stack([r["frame_tok"] for r in rows]),
            np.asarray([r["score"] for r in rows], F32))
