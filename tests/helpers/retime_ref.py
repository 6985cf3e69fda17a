"""numpy restatement of smtts_retime, written from include/smalltts_hip.h (not from the kernel): the stateful map, the segments, the
search in float64 and the cross-fade in three fp32 operations, free-running or teacher-forced (segment k takes q_{k-1} from a given
table, and its own q_k too, so that the overlap-add can be driven by a device's choices).  For every searched segment it returns the
float64 score of every candidate and E(l) = (H + 2) * 2^-24 * sum_i |x[c + i]| |x[p + l + i]|, which bounds the error of an fp32 dot
product of H terms in any order, with or without fma (gamma_H <= (H + 2) u for H <= 512, u = 2^-24): derived, not measured.

Also the signals and cases that tests/test_retime_cpu.py and tests/test_retime_gpu.py share."""
import numpy as np

SHAPES = ((32, 8), (240, 120))          # (hop, delta)
SPEEDS = (0.5, 0.8, 1.25, 2.0)
U = 2.0 ** -24


def window(hop):
    """The header leaves win to the caller; the tests use plans.retime_window's formula, restated."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(2 * hop, dtype=np.float64) + 0.5) / (2 * hop))).astype(np.float32)


class SrcMap:
    """M of the header for one row: clamped entries, evaluated at increasing t, the pair index never moves back."""

    def __init__(self, anchors, n_anchor, n, row_stride, out_stride):
        a = np.asarray(anchors, np.int64).reshape(-1, 2)
        self.m = int(min(max(int(n_anchor), 0), a.shape[0]))
        self.s = [min(max(int(v), 0), int(row_stride)) for v in a[:, 0]]
        self.d = [min(max(int(v), 0), int(out_stride)) for v in a[:, 1]]
        self.n, self.j = int(n), 0
        self.out_len = self.d[self.m - 1] if self.m >= 2 else 0

    def at(self, t):
        s, d, m = self.s, self.d, self.m
        while self.j + 1 < m and not (d[self.j + 1] > d[self.j] and d[self.j] <= t < d[self.j + 1]):
            self.j += 1
        j = self.j
        if j + 1 < m:
            r = s[j] + ((t - d[j]) * (s[j + 1] - s[j])) // (d[j + 1] - d[j])
        else:
            r = s[m - 1] + (t - d[m - 1])
        return min(max(r, 0), self.n)


def _take(x, n, s, cnt):
    """x[s, s + cnt) with +0.0 outside [0, n)."""
    out = np.zeros((cnt,), np.float32)
    lo, hi = max(s, 0), min(s + cnt, n)
    if hi > lo:
        out[lo - s: hi - s] = x[lo:hi]
    return out


def pick(lags, scores):
    """The header's argmax: the largest score, then the smaller |lag|, then the negative lag."""
    best = 0
    for i in range(1, len(lags)):
        if scores[i] > scores[best] or (scores[i] == scores[best] and (abs(lags[i]), lags[i]) < (abs(lags[best]), lags[best])):
            best = i
    return best


def retime_row(x, length, anchors, n_anchor, win, hop, delta, out_stride, q_forced=None, row_stride=None):
    """One row -> dict(out (out_len,) f32, q (K,) int64, out_len, K, p (K,) = M(k H), segments): segments[k] = None for a copy by the
    continuation rule (and for k = 0), else dict(p, c, lags, score, E, best): the candidates, their float64 scores and error bounds,
    the index of the header's argmax.  q_forced: a table of K entries whose q_{k-1} AND q_k replace the reference's own."""
    x = np.asarray(x, np.float32).reshape(-1)
    H, D = int(hop), int(delta)
    row_stride = x.shape[0] if row_stride is None else int(row_stride)
    n = min(max(int(length), 0), row_stride)
    M = SrcMap(anchors, n_anchor, n, row_stride, out_stride)
    out_len = M.out_len
    K = -(-out_len // H)
    out, q, segs = np.zeros((out_len,), np.float32), np.zeros((K,), np.int64), []
    w = np.asarray(win, np.float32)
    ps = np.zeros((K,), np.int64)
    for k in range(K):
        t0 = k * H
        cnt = min(H, out_len - t0)
        p = ps[k] = M.at(t0)
        if k == 0:
            q[0] = p if q_forced is None else int(q_forced[0])
            out[:cnt] = _take(x, n, int(q[0]), cnt)
            segs.append(None)
            continue
        c = int(q[k - 1] if q_forced is None else q_forced[k - 1]) + H
        tm = _take(x, n, c, H)
        if abs(c - p) <= D:
            qk, seg = c, None
        else:
            lags = [l for l in range(-D, D + 1) if 0 <= p + l <= n]
            t64, ta = tm.astype(np.float64), np.abs(tm.astype(np.float64))
            cand = [_take(x, n, p + l, H).astype(np.float64) for l in lags]
            with np.errstate(invalid="ignore"):
                score = np.asarray([float(np.dot(t64, v)) for v in cand])
                E = np.asarray([(H + 2) * U * float(np.dot(ta, np.abs(v))) for v in cand])
            score = np.where(np.isnan(score), -np.inf, score)   # the header: a NaN score counts as -inf
            best = pick(lags, score)
            qk, seg = p + lags[best], dict(p=p, c=c, lags=lags, score=score, E=E, best=best)
        if q_forced is not None:
            qk = int(q_forced[k])
        q[k] = qk
        if qk == c:
            out[t0: t0 + cnt] = tm[:cnt]
        else:
            new = _take(x, n, qk, H)
            out[t0: t0 + cnt] = ((tm * w[H:]).astype(np.float32) + (new * w[:H]).astype(np.float32)).astype(np.float32)[:cnt]
        segs.append(seg)
    return dict(out=out, q=q, out_len=out_len, K=K, p=ps, segments=segs)


def is_clear(res) -> bool:
    """Every searched segment's best score beats every other candidate's by more than E(best) + E(other)."""
    for seg in res["segments"]:
        if seg is None:
            continue
        b = seg["best"]
        margin = seg["score"][b] - seg["score"] - seg["E"][b] - seg["E"]
        margin[b] = np.inf
        if not (margin > 0).all():
            return False
    return True


def unclear(res) -> int:
    return sum(1 for seg in res["segments"] if seg is not None and not is_clear(dict(segments=[seg])))


def searched(res) -> int:
    return sum(seg is not None for seg in res["segments"])


# ---- the signals ---------------------------------------------------------------------------------------------------------------
def noise_signal(seed, n):
    """Gaussian noise smoothed by a 33-tap Hann kernel, peak 0.5."""
    rng = np.random.default_rng(seed)
    k = np.hanning(35)[1:-1]
    y = np.convolve(rng.standard_normal(n + 32), k / k.sum(), mode="valid")
    return (0.5 * y / np.abs(y).max()).astype(np.float32)


def voiced_signal(seed, n, sr=24000.0):
    """Eight harmonics of a 140 Hz tone with vibrato, a slow envelope and a 0.002 noise floor."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    phase = 2 * np.pi * 140.0 * t + 1.5 * np.sin(2 * np.pi * 5.0 * t)
    amps = 1.0 / (1.0 + np.arange(8)) * (0.5 + rng.random(8))
    y = sum(a * np.sin((h + 1) * phase + ph) for h, (a, ph) in enumerate(zip(amps, rng.random(8) * 2 * np.pi)))
    y = y * (0.6 + 0.4 * np.sin(2 * np.pi * 1.3 * t + 0.7))
    y = 0.5 * y / np.abs(y).max() + 0.002 * rng.standard_normal(n)
    return y.astype(np.float32)


SIGNALS = {"noise": noise_signal, "voiced": voiced_signal}
SEGMENTS = 50                                       # source segments of the uniform cases: n = 50 hop
CLEAR_SEEDS = {("noise", 32): 11, ("voiced", 32): 12, ("noise", 240): 13, ("voiced", 240): 14}   # chosen by running the reference


def uniform_case(name, hop, delta, speed, seed=None):
    n = SEGMENTS * hop
    x = SIGNALS[name](CLEAR_SEEDS[(name, hop)] if seed is None else seed, n)
    anchors = np.asarray([[0, 0], [n, int(round(n / speed))]], np.int64)
    return dict(x=x, len=n, anchors=anchors, hop=hop, delta=delta)


def clear_cases():
    """The cases the GPU's free-running test compares exactly: both signals at speed 1.25, at both shapes."""
    return {f"{name}-{hop}x{delta}": uniform_case(name, hop, delta, 1.25) for hop, delta in SHAPES for name in SIGNALS}


def wordlike_anchors(hop):
    """12 anchors with mixed slopes (between 1/2 and 2, one pause at 1/4 and one at 4), ending on a partial segment."""
    s = np.asarray([0, 3, 7, 10, 16, 18, 24, 27, 33, 36, 41, 45], np.int64) * hop
    r = [2.0, 1.0, 0.5, 1.5, 0.25, 1.0, 4.0, 0.75, 1.25, 0.6, 1.0]
    d = [0]
    for i, rate in enumerate(r):
        d.append(d[-1] + max(1, int(round(int(s[i + 1] - s[i]) / rate))))
    d[-1] += hop // 3 + 1                                        # ... so that the last segment is partial
    return np.stack([s, np.asarray(d, np.int64)], axis=1)


def teacher_cases():
    """Every case of the teacher-forced GPU test, by name."""
    out = {}
    for hop, delta in SHAPES:
        tag = f"{hop}x{delta}"
        for name in SIGNALS:
            for sp in SPEEDS:
                out[f"{name}-{tag}-speed{sp}"] = uniform_case(name, hop, delta, sp)
        n = 45 * hop
        out[f"wordlike-{tag}"] = dict(x=voiced_signal(21, n + 40), len=n, anchors=wordlike_anchors(hop), hop=hop, delta=delta)
        burst = np.zeros((40 * hop,), np.float32)
        burst[15 * hop: 22 * hop] = noise_signal(22, 7 * hop)
        out[f"burst-{tag}"] = dict(x=burst, len=burst.size, anchors=np.asarray([[0, 0], [burst.size, int(burst.size / 1.6)]], np.int64),
                                   hop=hop, delta=delta)
        short = hop - 5
        out[f"short-{tag}"] = dict(x=noise_signal(23, hop + 9), len=short, anchors=np.asarray([[0, 0], [short, 2 * short]], np.int64),
                                   hop=hop, delta=delta)
        out[f"empty-{tag}"] = dict(x=noise_signal(24, hop), len=0, anchors=np.asarray([[0, 0], [0, 3 * hop + 1]], np.int64),
                                   hop=hop, delta=delta)
        n = 20 * hop
        out[f"partial-{tag}"] = dict(x=voiced_signal(25, n), len=n, anchors=np.asarray([[0, 0], [n, int(n / 0.7) + hop // 2 + 1]], np.int64),
                                     hop=hop, delta=delta)
    return out
