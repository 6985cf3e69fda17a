"""numpy restatement of smtts_pitch, written from include/smalltts_hip.h (not from the kernels): the scores in float64 with a derived
error bound per element, and the path (local costs, transitions, recurrence, end, back pointers, peak) on a GIVEN fp32 S in the
header's separately rounded fp32 operations, so that it can be driven by a device's own scores and then has to agree bit for bit.

The score bound, first order in u = 2^-24 and g = (win + 2) u (gamma_win <= (win + 2) u for win <= 2048: an fp32 sum of win products in
any order, with or without fma):  |S_dev - S_64| <= 2 * (g * sum_i |x_i y_i| / den  +  |S| * (g + 4 u)),  den = sqrt(e0 e + bias).
The first term covers r.  The second covers the two energies (g each, relative), their product (u), the add of bias (u), the root
(which halves what is under it: g + u, plus its own u) and the divide (u): g + 3 u, rounded up to g + 4 u.  hipcc's sqrtf and divide
are correctly rounded by default.  The factor 2 is the ONE safety factor of the bound (second-order terms, and the rounding of S_64 to
fp32 where the two are compared as fp32).  No constant comes from a GPU run.

Also the signals, the shapes and the conditions that tests/test_pitch_cpu.py and tests/test_pitch_gpu.py share, and the broken copies
of the path that show the conditions can fail."""
import numpy as np

U = 2.0 ** -24
SR = 24000


class Shape:
    """The numbers of one call: hop, win, lmin, lmax and the costs; tab = plans.pitch_tables' formula, restated."""

    def __init__(self, hop=240, win=480, lmin=60, lmax=400, floor_pow=1e-6, tilt=0.1, c_unv=0.55, w_jump=0.35, w_switch=0.3):
        self.hop, self.win, self.lmin, self.lmax = hop, win, lmin, lmax
        self.L = lmax - lmin + 1
        self.bias = np.float32((win * floor_pow) ** 2)
        self.c_unv, self.w_jump, self.w_switch = np.float32(c_unv), np.float32(w_jump), np.float32(w_switch)
        l = np.arange(lmin, lmax + 1, dtype=np.float64)
        self.tab = np.stack([np.log2(l), 1.0 - tilt * (l - lmin) / (lmax - lmin)]).astype(np.float32)
        self.reach = win + lmax                                  # a frame at s reads x[s, s + reach)

    def frames(self, n):
        return -(-int(n) // self.hop)


DEFAULT = Shape()
TINY = Shape(hop=16, win=64, lmin=8, lmax=40)                    # L = 33: no multiple of 4 or 64
WIDE = Shape(hop=16, win=32, lmin=2, lmax=1024)                  # L = 1023: the most states, one share, one wave per 64 of them
SHAPES = {"default": DEFAULT, "tiny": TINY, "wide": WIDE}


def _clamped(x, length, row_stride=None):
    x = np.asarray(x, np.float32).reshape(-1)
    row_stride = x.size if row_stride is None else int(row_stride)
    n = min(max(int(length), 0), row_stride)
    return x, n


def scores(x, length, P, row_stride=None, bias=None):
    """One row -> (S (F, L) float64, E (F, L) float64: the bound of the module docstring).  x[i] outside [0, n) reads as +0.0."""
    x, n = _clamped(x, length, row_stride)
    F = P.frames(n)
    bias = float(P.bias if bias is None else bias)
    S, E = np.zeros((F, P.L)), np.zeros((F, P.L))
    g = (P.win + 2) * U
    xp = np.zeros(((F - 1) * P.hop + P.reach if F else 0,), np.float64)
    xp[:min(n, xp.size)] = x[:min(n, xp.size)]
    for f in range(F):
        seg = xp[f * P.hop: f * P.hop + P.reach]
        t = seg[:P.win]
        w = np.lib.stride_tricks.sliding_window_view(seg, P.win)[P.lmin: P.lmax + 1]      # (L, win): the candidates
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            r, e, e0 = w @ t, (w * w).sum(axis=1), float(t @ t)
            den = np.sqrt(e0 * e + bias)
            S[f] = r / den
            E[f] = 2.0 * (g * (np.abs(w) @ np.abs(t)) / den + np.abs(S[f]) * (g + 4 * U))
    return S, E


def tables(tab, L):
    """lg and tilt as the header clamps them: lg into [0, 16], tilt into [0, 2], a NaN reads as 0."""
    t = np.asarray(tab, np.float32).reshape(2, L)
    fix = lambda v, hi: np.clip(np.where(np.isnan(v), np.float32(0), v), np.float32(0), np.float32(hi)).astype(np.float32)
    return fix(t[0], 16), fix(t[1], 2)


def path(S, P, ties="smallest", tab=None, w_switch=None):
    """The header's path through a given fp32 S (F, L) -> (lag (F,) int32, peak (F, 3) fp32).  Every operation is one fp32 numpy
    operation, so each is rounded on its own.  ties="largest" and w_switch=0 are the broken copies."""
    S = np.asarray(S, np.float32)
    F, L = S.shape
    f32 = np.float32
    lg, tilt = tables(P.tab if tab is None else tab, L)
    w_sw = P.w_switch if w_switch is None else f32(w_switch)
    with np.errstate(invalid="ignore", over="ignore"):
        T = np.zeros((L + 1, L + 1), f32)                          # T[j', j]
        T[1:, 1:] = P.w_jump * np.abs(lg[None, :] - lg[:, None])   # fmul(w_jump, fabsf(fsub(lg[j-1], lg[j'-1])))
        T[0, 1:] = w_sw
        T[1:, 0] = w_sw

        def loc(f):
            v = f32(1) - S[f] * tilt                               # fsub(1, fmul(S, tilt))
            return np.concatenate([[P.c_unv], np.where(np.isnan(v), f32(np.inf), v)]).astype(f32)

        def argmin(c, axis=0):                                     # the smallest index among the minima; a NaN never wins
            c = np.where(np.isnan(c), f32(np.inf), c)
            if ties == "smallest":
                return np.argmin(c, axis=axis)
            return c.shape[axis] - 1 - np.argmin(np.flip(c, axis=axis), axis=axis)

        lag, peak = np.zeros((F,), np.int32), np.zeros((F, 3), f32)
        if F == 0:
            return lag, peak
        D = loc(0)
        bp = np.zeros((F, L + 1), np.int64)
        for f in range(1, F):
            cand = (D[:, None] + T).astype(f32)                    # fadd(D[f-1][j'], trans(j', j))
            bp[f] = argmin(cand)
            best = np.where(np.isnan(cand), f32(np.inf), cand)[bp[f], np.arange(L + 1)]
            D = (loc(f) + best).astype(f32)
        q = int(np.argmin(np.where(np.isnan(D), f32(np.inf), D)))  # the end: always the smallest j among the minima
        for f in range(F - 1, -1, -1):
            if q > 0:
                c = q - 1
                lag[f] = P.lmin + c
                peak[f] = (S[f, c - 1] if c > 0 else S[f, c], S[f, c], S[f, c + 1] if c + 1 < L else S[f, c])
            q = int(bp[f, q])
    return lag, peak


def track(x, length, P, **broken):
    """Free-running: the float64 scores rounded to fp32, then the path -> (lag, peak, S32)."""
    bias = broken.pop("bias", None)
    S, _E = scores(x, length, P, bias=bias)
    S32 = S.astype(np.float32)
    lag, peak = path(S32, P, **broken)
    return lag, peak, S32


# ---- the signals ---------------------------------------------------------------------------------------------------------------------
def tone(f0, n, start, stop, hole=None, seed=0, floor=1e-4, sr=SR):
    """Four harmonics (1, 1/2, 1/3, 1/4) of f0 on [start, stop), silent outside and inside `hole` = (a, b), peak 0.5, on a noise floor."""
    t = np.arange(n) / sr
    y = sum(np.sin(2 * np.pi * (k + 1) * f0 * t + 0.7 * k) / (k + 1) for k in range(4))
    y = 0.5 * y / np.abs(y).max()
    gate = np.zeros((n,))
    gate[start:stop] = 1.0
    if hole is not None:
        gate[hole[0]: hole[1]] = 0.0
    return (y * gate + floor * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def periodic(period, n, start, stop, seed=0, floor=1e-4):
    """The same at the tiny shape: four harmonics of a period given in samples."""
    return tone(SR / period, n, start, stop, None, seed, floor)


def white(seed, n, amp=0.1):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


TONES = (65.0, 100.0, 220.0, 390.0)
TONE_N, TONE_ON, TONE_OFF, TONE_HOLE = 36000, 3600, 32400, (16800, 19200)   # 1.5 s: silent ends of 150 ms, a hole of 100 ms
TINY_PERIODS = (9, 13, 20, 31, 38)
TINY_N, TINY_ON, TINY_OFF = 1600, 240, 1360


def tone_case(f0):
    return tone(f0, TONE_N, TONE_ON, TONE_OFF, TONE_HOLE, seed=int(f0))


def tiny_case(period):
    return periodic(period, TINY_N, TINY_ON, TINY_OFF, seed=period)


def inside(P, n, spans):
    """The frames whose whole reach [s, s + win + lmax) lies inside one of `spans` -> a boolean (F,)."""
    s = np.arange(P.frames(n)) * P.hop
    return np.any([(s >= a) & (s + P.reach <= b) for a, b in spans], axis=0)


def check_tone(lag, P, n, on, off, hole, period):
    """The conditions of a tone case: every frame whose reach lies inside the tone is voiced within one step of the integer lag grid of
    the period; every frame whose reach lies in silence is unvoiced.  -> (tone frames, silent frames) checked."""
    lag = np.asarray(lag)[:P.frames(n)]
    tone_spans = [(on, off)] if hole is None else [(on, hole[0]), (hole[1], off)]
    quiet_spans = [(0, on), (off, n + P.reach)] + ([] if hole is None else [hole])   # behind n everything reads as zero
    t, q = inside(P, n, tone_spans), inside(P, n, quiet_spans)
    assert t.sum() >= 3 and q.sum() >= 3, (t.sum(), q.sum())
    assert (lag[t] > 0).all(), ("unvoiced inside the tone", period, lag[t])
    assert (np.abs(lag[t] - period) <= 1.0).all(), ("lag off the period", period, lag[t])
    assert (lag[q] == 0).all(), ("voiced in silence", period, lag[q])
    return int(t.sum()), int(q.sum())


# ---- the retime / pitch yardstick -----------------------------------------------------------------------------------------
YARD_SPEEDS = (0.8, 1.25)
D_REF = 2                                   # the reference's own worst lag deviation (tests/test_pitch_cpu.py measures and asserts it)


def yardstick_pairs(P, n_in, n_out, speed):
    """Output frame f is compared with input frame round(f * speed); inner frames only: the reach of both lies inside its signal, and
    the first two frames of each are left out."""
    fo = np.arange(2, P.frames(n_out))
    fi = np.rint(fo * speed).astype(np.int64)
    ok = (fi >= 2) & (fo * P.hop + P.reach <= n_out) & (fi * P.hop + P.reach <= n_in)
    return fo[ok], fi[ok]


def yardstick(lag_in, lag_out, P, n_in, n_out, speed):
    """-> (the worst lag deviation over the compared frames, how many of them differ in voicing or are unvoiced, how many pairs)."""
    fo, fi = yardstick_pairs(P, n_in, n_out, speed)
    a, b = np.asarray(lag_in)[fi], np.asarray(lag_out)[fo]
    unv = int(((a == 0) | (b == 0)).sum())
    both = (a > 0) & (b > 0)
    return (int(np.abs(a[both] - b[both]).max()) if both.any() else 0), unv, int(fo.size)
