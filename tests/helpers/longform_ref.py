"""Numpy restatements of the long-form kernels' definitions (include/smalltts_hip.h smtts_stitch), shared by the CPU test that pins
them against a naive loop and the GPU tests that hold the kernels to them bit for bit."""
import numpy as np


def pcm16_numpy(x: np.ndarray) -> np.ndarray:
    """smtts_pcm16: clamp to [-1, 1], times 32767 in fp32, round to nearest even."""
    v = np.clip(np.asarray(x, np.float32), np.float32(-1.0), np.float32(1.0)) * np.float32(32767.0)
    return np.rint(v).astype(np.int16)


def stitch_numpy(out: np.ndarray, audio: np.ndarray, lens, offsets, fade: np.ndarray) -> np.ndarray:
    """Writes rows audio[b, 0, :lens[b]] faded by the table `fade` (fp32, F entries, F may be 0) into out (1-D fp32 or int16)
    at offsets[b], vectorised per row; everything else in `out` is left as it is."""
    fade = np.asarray(fade, np.float32)
    F = fade.shape[0]
    for b, (n, o) in enumerate(zip(lens, offsets)):
        n, o = int(n), int(o)
        row = np.array(audio[b, 0, :n], np.float32)
        Fb = min(F, n // 2)
        if Fb:
            row[:Fb] = row[:Fb] * fade[:Fb]
            row[n - Fb:] = row[n - Fb:] * fade[:Fb][::-1]
        out[o:o + n] = pcm16_numpy(row) if out.dtype == np.int16 else row
    return out


def stitch_naive(out: np.ndarray, audio: np.ndarray, lens, offsets, fade: np.ndarray) -> np.ndarray:
    """The same definition, one sample at a time, straight from its wording."""
    F = len(fade)
    for b in range(len(lens)):
        n = int(lens[b])
        Fb = min(F, n // 2)
        for i in range(n):
            v = np.float32(audio[b, 0, i])
            if i < Fb:
                v = np.float32(v * np.float32(fade[i]))
            elif i >= n - Fb:
                v = np.float32(v * np.float32(fade[n - 1 - i]))
            if out.dtype == np.int16:
                c = np.float32(min(max(v, np.float32(-1.0)), np.float32(1.0))) * np.float32(32767.0)
                out[int(offsets[b]) + i] = np.int16(np.rint(np.float32(c)))
            else:
                out[int(offsets[b]) + i] = v
    return out


# the ragged cases of the stitch tests: (hop, frames per row of each batch, fade length F, gap in samples)
STITCH_CASES = [
    (16, [[3, 1, 5], [2, 4]], 6, 7),        # a row of one hop (len = 16 > 2 F: full fade), ragged, an odd gap (unaligned offsets)
    (16, [[1, 2], [1]], 0, 4),              # F = 0: a pure copy
    (8, [[1, 3, 2], [1, 1]], 20, 0),        # F > len // 2 on every row (the fades meet in the middle), gap 0
    (12, [[4]], 5, 3),                      # one row
    (3200, [[2, 1], [1, 3, 1]], 120, 2880),  # the product's hop, fade (5 ms) and gap (120 ms)
]


def stitch_case(hop, batches, F, gap, seed=0):
    """-> (list of (audio (B,1,hop*Nmax) fp32, lens, offsets) per batch, fade (F,) fp32, total samples S)."""
    g = np.random.default_rng(seed)
    fade = (0.5 - 0.5 * np.cos(np.pi * (np.arange(F, dtype=np.float64) + 0.5) / max(F, 1))).astype(np.float32)[:F]
    out, pos = [], 0
    for ns in batches:
        audio = (g.standard_normal((len(ns), 1, hop * max(ns))) * 0.6).astype(np.float32)   # some samples beyond +-1: the PCM clamp works
        lens, offs = [hop * n for n in ns], []
        for n in lens:
            offs.append(pos)
            pos += n + gap
        out.append((audio, lens, offs))
    return out, fade, pos - gap
