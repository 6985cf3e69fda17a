"""numpy restatement of smtts_watermark and smtts_watermark_detect, written from include/smalltts_hip.h (not from the kernels): the chips
through oracle.philox, the embedder as a float32 loop that reproduces the device bit for bit, the detector in fp64 with the
magnitudes its fp32 error bounds need, and the speech-like test signal.  tests/test_watermark_cpu.py holds it to itself (chunked
against whole) and to the statistics the scheme promises; tests/test_watermark_gpu.py holds the kernels to it."""
import numpy as np

from oracle import philox

STREAM_ID = 0x574D4B31   # 'WMK1'
HIST = 127
EPS = 1e-8
U = 2.0 ** -24           # unit roundoff of fp32


# ---- chips ---------------------------------------------------------------------------------------------------------------------
def chips(i0: int, n: int, key: int) -> np.ndarray:
    """c[i0 .. i0 + n) as int8 +1 / -1."""
    if n <= 0:
        return np.zeros(0, np.int8)
    g0, g1 = i0 >> 7, (i0 + n - 1) >> 7
    g = np.arange(g0, g1 + 1, dtype=np.uint64)
    ctr = np.stack([g & philox.MASK, g >> np.uint64(32), np.full(len(g), STREAM_ID, np.uint64), np.zeros(len(g), np.uint64)],
                   -1).astype(np.uint32)
    w = philox.philox4x32_10(ctr, int(key) & (2 ** 64 - 1))                                  # (G, 4): word (i >> 5) & 3 of group i >> 7
    bits = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(-1)   # ... bit i & 31
    a = i0 - (g0 << 7)
    return np.where(bits[a: a + n] != 0, 1, -1).astype(np.int8)


# ---- embedder: float32, exact -----------------------------------------------------------------------------------------------------
def _envelope(blocks: np.ndarray) -> np.ndarray:
    """R of (K, 64) float32 blocks: the sequential chain over j, every product and every sum rounded to float32."""
    acc = np.zeros(len(blocks), np.float32)
    for j in range(64):
        sq = blocks[:, j] * blocks[:, j]
        acc = acc + sq
    return np.sqrt(acc * np.float32(0.015625))


def embed(x: np.ndarray, key: int, strength: float, start: int = 0, hist: np.ndarray = None) -> np.ndarray:
    """The marked samples [start, start + len(x)) of a stream whose samples there are x and whose 127 samples in front are `hist`
    (oldest first; zeros: the slot of a fresh stream)."""
    x = np.asarray(x, np.float32)
    n = len(x)
    if n == 0:
        return x.copy()
    hist = np.zeros(HIST, np.float32) if hist is None else np.asarray(hist, np.float32)
    assert hist.shape == (HIST,)
    ext = np.concatenate([hist, x])                      # ext[q] = stream sample start - 127 + q
    k_lo, k_hi = start >> 6, (start + n - 1) >> 6
    ks = np.arange(k_lo, k_hi + 1)
    amp = np.zeros(len(ks), np.float32)
    need = ks > 0                                        # A[0] = 0
    if need.any():
        first = (ks[need] - 1) * 64 - (start - HIST)     # block k - 1 in ext: >= 0 because 64 (k - 1) >= i - 127 for every i of block k
        assert first.min() >= 0
        blocks = ext[first[:, None] + np.arange(64)[None, :]]
        amp[need] = np.float32(strength) * _envelope(blocks)
    i = start + np.arange(n)
    a = amp[(i >> 6) - k_lo]
    c = chips(start, n, key)
    return np.where(c > 0, x + a, x - a).astype(np.float32)


class Stream:
    """One stream marked in chunks: push(chunk) -> the marked chunk; .hist is the slot's content after the call (the last 127 INPUT
    samples, oldest first; zeros in front of a young stream); .n the samples seen.  start: the position the stream claims to begin
    at (a zero slot with n_before = start)."""

    def __init__(self, key: int, strength: float, start: int = 0):
        self.key, self.strength, self.n = int(key), float(strength), int(start)
        self.hist = np.zeros(HIST, np.float32)

    def push(self, chunk: np.ndarray) -> np.ndarray:
        chunk = np.asarray(chunk, np.float32)
        y = embed(chunk, self.key, self.strength, self.n, self.hist)
        self.hist = np.concatenate([self.hist, chunk])[-HIST:]
        self.n += len(chunk)
        return y


# ---- detector: fp64 ------------------------------------------------------------------------------------------------------------------
def _shift(y: np.ndarray, d: int) -> np.ndarray:
    """s[j] = y[j + d], zeros outside."""
    n = len(y)
    s = np.zeros(n)
    if d >= 0:
        s[: max(0, n - d)] = y[d:]
    else:
        s[-d:] = y[: n + d]
    return s


def _win_sum(a: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """s[j] = sum_{m = j + lo .. j + hi} a[m], zeros outside (a >= 0: prefix sums lose nothing that matters in fp64)."""
    n = len(a)
    c = np.concatenate([[0.0], np.cumsum(a)])
    j = np.arange(n)
    return c[np.clip(j + hi + 1, 0, n)] - c[np.clip(j + lo, 0, n)]


def detect_u(y: np.ndarray):
    """u of the whole signal y in fp64 -> (u, bound): bound[j] >= |fp32 u[j] - u[j]| for the device's order of operations.

    The bound, operation by operation, in units of U = 2^-24 relative to the magnitudes named (first order; rn = one rounding):
      d4 = ((y[j-2] + y[j+2]) - 4 (y[j-1] + y[j+1])) + 6 y[j]: y[j+-2] and y[j+-1] pass three roundings (the pair's add, the subtract,
           the last add; x 4 is exact), y[j] two (x 6, the last add):              |err d4| <= 3 U M4,  M4 = sum |coefficient y|
      d2 = (y[m-1] + y[m+1]) - 2 y[m]: two roundings:                               |err d2| <= 2 U M2,  M2 = |y[m-1]| + |y[m+1]| + 2 |y[m]|
      d2^2: 2 |d2| |err d2| + one rn:                                              |err| <= U (4 |d2| M2 + d2^2)
      v = (1/64) chain of 64: 63 adds, each <= U x the final sum; x 1/64 exact:    |err v| <= U ((1/64) sum (4 |d2| M2 + d2^2) + 63 v)
      r = sqrt((1/64) chain of 64 squares): radicand 1 + 63 rn relative, halved by the root, + 1 rn: |err r| <= 33 U r
      D = v + 1e-8f: + one rn; 1e-8f itself is the fp32 constant, which the restatement uses too:    |err D| <= |err v| + U D
      u = (d4 r) / D: two rn:   |err u| <= (3 U M4 r + |d4| 33 U r) / D + |u| |err D| / D + 2 U |u|
    Contraction into fma only removes roundings.  Second order: the function asserts that every relative term is below 2^-10 (the
    test signals' are below 2^-11), where the products of (1 + e) factors stay within 1 % of first order: x 1.01.  2^-100 absolute
    covers fp32 underflow of squares.  The fp64 restatement's own error (2^-53 on the same magnitudes) is 2^-29 of the bound."""
    y = np.asarray(y, np.float32).astype(np.float64)
    n = len(y)
    if n == 0:
        return np.zeros(0), np.zeros(0)
    a = np.abs(y)
    ym2, ym1, yp1, yp2 = _shift(y, -2), _shift(y, -1), _shift(y, 1), _shift(y, 2)
    d2 = ym1 - 2 * y + yp1
    d4 = ym2 - 4 * ym1 + 6 * y - 4 * yp1 + yp2
    M2 = _shift(a, -1) + 2 * a + _shift(a, 1)
    M4 = _shift(a, -2) + 4 * _shift(a, -1) + 6 * a + 4 * _shift(a, 1) + _shift(a, 2)
    r = np.sqrt(_win_sum(y * y, -96, -33) / 64)
    v = _win_sum(d2 * d2, -32, 31) / 64
    eps = float(np.float32(EPS))
    D = v + eps
    u = d4 * r / D
    ev = _win_sum(4 * np.abs(d2) * M2 + d2 * d2, -32, 31) / 64 + 63 * v          # in units of U
    eD = ev + D
    assert (eD / D).max() * U < 2.0 ** -10, "the first-order bound's precondition"
    bound = U * ((3 * M4 * r + 33 * np.abs(d4) * r) / D + np.abs(u) * eD / D + 2 * np.abs(u)) * 1.01 + 2.0 ** -100
    return u, bound


def correlate(u: np.ndarray, key: int, o_lo: int, n_off: int) -> np.ndarray:
    """T(o_lo + k) for k < n_off, in fp64."""
    u = np.asarray(u, np.float64)
    n = len(u)
    c = chips(o_lo, n + n_off, key).astype(np.float64)
    return np.array([float(np.dot(u, c[k: k + n])) for k in range(n_off)])


def detect(y: np.ndarray, key: int, o_lo: int = 0, n_off: int = 1):
    """-> dict(u, bound, den, T (n_off), z (n_off), best_off, best_z, sum_abs_u): the detector on the whole signal y in fp64."""
    u, bound = detect_u(y)
    den = float(np.sum(u * u))
    T = correlate(u, key, o_lo, n_off)
    z = T / np.sqrt(den) if den > 0 else np.zeros(n_off)
    k = int(np.argmax(T))
    return {"u": u, "bound": bound, "den": den, "T": T, "z": z, "best_off": o_lo + k, "best_z": float(z[k]),
            "sum_abs_u": float(np.sum(np.abs(u)))}


def t_bound(sum_abs_u: float, n: int) -> float:
    """|device T(o) - exact sum of the device's own u| <= (1024 + n_tiles + 2) 2^-24 sum |u_j|: a tile's chain is at most 1024 adds,
    the running total n_tiles more."""
    return (1024 + -(-n // 1024) + 2) * U * sum_abs_u


def den_bound(sum_sq_u: float, n: int) -> float:
    """The tree's analogue: a u^2 passes 1 rounding (the square), 4 (a thread's chain of four), 8 (the tree), ceil(n_tiles / 256)
    (a thread's chain over tiles) and 8 (the second tree): (21 + ceil(n_tiles / 256) + 2) 2^-24 sum u_j^2."""
    nt = -(-n // 1024)
    return (21 + -(-nt // 256) + 2) * U * sum_sq_u


# ---- the speech-like signal -------------------------------------------------------------------------------------------------------
def speechlike(seconds: float = 10.0, seed: int = 0, rate: int = 24000) -> np.ndarray:
    """A 120 Hz pulse train through three formant resonators in cascade (700 / 1200 / 2600 Hz), a 3 Hz syllabic envelope with gated
    pauses, and weak high-passed noise bursts: float32 with peak 0.5."""
    n = int(round(seconds * rate))
    rng = np.random.default_rng(seed)
    L = 4096
    h = np.zeros(L)
    h[0] = 1.0
    t = np.arange(L)
    for f, bw in ((700.0, 90.0), (1200.0, 110.0), (2600.0, 160.0)):
        rr = np.exp(-np.pi * bw / rate)
        th = 2 * np.pi * f / rate
        res = rr ** t * np.sin(th * (t + 1)) / np.sin(th)            # impulse response of 1 / (1 - 2 r cos(th) z^-1 + r^2 z^-2)
        h = np.convolve(h, res)[:L]
    x = np.zeros(n + L)
    period = rate // 120
    for p in range(0, n, period):
        x[p: p + L] += h * (1.0 + 0.05 * rng.standard_normal())
    x = x[:n]
    tt = np.arange(n) / rate
    env = 0.5 - 0.5 * np.cos(2 * np.pi * 3.0 * tt)
    env = np.where(env > 0.15, env, 0.0)                             # gated pauses
    bursts = np.diff(rng.standard_normal(n + 1)) * (np.sin(2 * np.pi * 1.3 * tt + 1.0) > 0.8)
    x = x / np.abs(x).max() * env + 0.004 * bursts
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def pcm16_round(y: np.ndarray) -> np.ndarray:
    """smtts_pcm16's value as the detector sees it after a WAV: clamp, x 32767, round to nearest even, / 32767."""
    s = np.rint(np.clip(np.asarray(y, np.float32), np.float32(-1), np.float32(1)) * np.float32(32767.0)).astype(np.int16)
    return s.astype(np.float32) / np.float32(32767.0)
