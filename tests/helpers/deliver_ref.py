"""numpy restatement of smtts_deliver, written from include/smalltts_hip.h (not from the kernel): fp64 sums on the f32 bank, the emission
rule, the carried history and the three encoders.  tests/test_deliver_cpu.py holds it to brute force, to audioop's codes
(tests/golden/g711_codes.npz) and to itself (chunked against whole); tests/test_deliver_gpu.py holds the kernel to it."""
import numpy as np


def frames(m: int, width: int, down: int) -> int:
    """F(m) = max(0, (m - width) / down)."""
    return max(0, (m - width) // down)


def count(n_before: int, length: int, last: bool, up: int, down: int, width: int) -> int:
    n = n_before + length
    return (-(-up * n // down) if last else up * frames(n, width, down)) - up * frames(n_before, width, down)


def count_brute(n_before: int, length: int, last: bool, up: int, down: int, width: int) -> int:
    """The definition, frame by frame: frame f is emitted with the first chunk end m at which all its inputs
    x[f * down - width .. f * down - width + klen) have arrived (or may be taken as zeros: the stream has ended)."""
    klen = 2 * width + down
    arrived = lambda m: sum(1 for f in range(0, m // down + 2) if f * down - width + klen <= m)
    n = n_before + length
    before = up * arrived(n_before)
    return (-(-up * n // down) if last else up * arrived(n)) - before


def resample_samples(x: np.ndarray, ended: bool, bank: np.ndarray, down: int, width: int, o_lo: int, o_hi: int):
    """Samples [o_lo, o_hi) of the resampled stream x (everything seen so far), in fp64, and sum_k |x_k bank_k| for the error bound.
    Indices below 0 enter as zeros; indices at or past len(x) too (they are only reached once the stream has ended)."""
    up, klen = bank.shape
    x = np.asarray(x, np.float32).astype(np.float64)
    b64 = bank.astype(np.float64)
    y = np.zeros(max(0, o_hi - o_lo))
    mag = np.zeros_like(y)
    for i, o in enumerate(range(o_lo, o_hi)):
        f, p = divmod(o, up)
        s0 = f * down - width
        idx = np.arange(s0, s0 + klen)
        ok = (idx >= 0) & (idx < len(x))
        assert ended or ok[idx >= 0].all(), "a frame was emitted before its inputs arrived"
        w = np.zeros(klen)
        w[ok] = x[idx[ok]]
        y[i] = float(np.dot(w, b64[p]))
        mag[i] = float(np.dot(np.abs(w), np.abs(b64[p])))
    return y, mag


def deliver_whole(x: np.ndarray, bank: np.ndarray, down: int, width: int):
    """n_before = 0, len = n, last = 1: (y fp64, mag) of ceil(up * n / down) samples."""
    up = bank.shape[0]
    return resample_samples(x, True, bank, down, width, 0, -(-up * len(x) // down))


class Stream:
    """One stream delivered in chunks: push(chunk, last) -> (y fp64, mag) of the samples that call emits; .hist is the slot's content
    after the call (f32, the last H = klen - 1 samples of x[0 .. n), oldest first; zeros in front of a young stream)."""

    def __init__(self, bank: np.ndarray, down: int, width: int):
        self.bank, self.down, self.width = bank, int(down), int(width)
        self.up, self.klen = bank.shape
        assert self.klen == 2 * self.width + self.down
        self.x = np.zeros(0, np.float32)
        self.hist = np.zeros(self.klen - 1, np.float32)

    def advance(self, chunk: np.ndarray, last: bool):
        """Takes the chunk in: -> (o_lo, o_hi), the samples this call emits; .hist moves on."""
        nb = len(self.x)
        chunk = np.asarray(chunk, np.float32)
        self.x = np.concatenate([self.x, chunk])
        n = len(self.x)
        H = self.klen - 1
        self.hist = np.concatenate([self.hist, chunk])[-H:] if H else self.hist
        o_lo = self.up * frames(nb, self.width, self.down)
        o_hi = -(-self.up * n // self.down) if last else self.up * frames(n, self.width, self.down)
        return o_lo, o_hi

    def push(self, chunk: np.ndarray, last: bool):
        o_lo, o_hi = self.advance(chunk, last)
        return resample_samples(self.x, bool(last), self.bank, self.down, self.width, o_lo, o_hi)


# ---- encoders ------------------------------------------------------------------------------------------------------------------
def pcm16(x: np.ndarray) -> np.ndarray:
    """smtts_pcm16: clamp to [-1, 1], x 32767 (one fp32 multiply), round to nearest even."""
    v = np.clip(np.asarray(x, np.float32), np.float32(-1.0), np.float32(1.0)) * np.float32(32767.0)
    return np.rint(v).astype(np.int16)


def _seg(v: np.ndarray, first_end: int) -> np.ndarray:
    ends = [(first_end + 1) * (1 << i) - 1 for i in range(8)]
    return sum((v > e).astype(np.int32) for e in ends)


def mulaw(s: np.ndarray) -> np.ndarray:
    v = np.asarray(s, np.int16).astype(np.int32) >> 2
    mask = np.where(v < 0, 0x7F, 0xFF)
    v = np.minimum(np.abs(v), 8159) + 33
    g = _seg(v, 0x3F)
    gg = np.minimum(g, 7)
    code = np.where(g >= 8, 0x7F ^ mask, ((gg << 4) | ((v >> (gg + 1)) & 15)) ^ mask)
    return code.astype(np.uint8)


def alaw(s: np.ndarray) -> np.ndarray:
    v = np.asarray(s, np.int16).astype(np.int32) >> 3
    mask = np.where(v < 0, 0x55, 0xD5)
    v = np.where(v < 0, -v - 1, v)
    g = _seg(v, 0x1F)
    gg = np.minimum(g, 7)
    code = np.where(g >= 8, 0x7F ^ mask, ((gg << 4) | ((v >> np.where(gg < 2, 1, gg)) & 15)) ^ mask)
    return code.astype(np.uint8)


def encode(y32: np.ndarray, enc: int) -> np.ndarray:
    """enc 0 f32, 1 pcm16, 2 mu-law, 3 A-law, applied to an f32 result."""
    y32 = np.asarray(y32, np.float32)
    return (y32, pcm16(y32), mulaw(pcm16(y32)), alaw(pcm16(y32)))[enc] if enc else y32


def mulaw_decode(c: np.ndarray) -> np.ndarray:
    u = ~np.asarray(c, np.uint8).astype(np.int32) & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84)


def alaw_decode(c: np.ndarray) -> np.ndarray:
    a = np.asarray(c, np.uint8).astype(np.int32) ^ 0x55
    seg = (a & 0x70) >> 4
    t = (a & 15) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t)


def fp32_bound(mag: np.ndarray, klen: int) -> np.ndarray:
    """|fp32 sum in any order - exact| <= (klen + 2) * 2^-24 * sum_k |x_k bank_k| per sample (klen products, klen adds, first order)."""
    return (klen + 2) * 2.0 ** -24 * mag
