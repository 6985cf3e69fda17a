"""Numpy restatements of the endpoint kernels' definitions (include/smalltts_hip.h smtts_endpoints, smtts_stitch_seg),
shared by the CPU test that pins them against naive loops and the GPU tests that hold the kernels to them.

A parameter set `p` is the dict Endpointing.kernel_params() returns: W, rel_pow, floor_pow, min_run, lead, tail, target_rms,
peak_limit, max_gain.  `dt` is np.float32 (the kernel's arithmetic, one rounding per operation) or np.float64 (the reference the
kernel's energies are held to); the fp32-rounded parameters are used as they are in both."""
import numpy as np

from tests.helpers.longform_ref import pcm16_numpy

DEFAULT_PARAMS = {"W": 240, "rel_pow": np.float32(1e-4), "floor_pow": np.float32(1e-8), "min_run": 3, "lead": 720, "tail": 1440,
                  "target_rms": np.float32(0.0), "peak_limit": np.float32(10.0 ** (-1 / 20)), "max_gain": np.float32(10.0)}


def params(**kw):
    p = dict(DEFAULT_PARAMS)
    p.update(kw)
    return p


def frame_counts(n: int, W: int) -> np.ndarray:
    F = (n + W - 1) // W
    return np.minimum(n, (np.arange(F, dtype=np.int64) + 1) * W) - np.arange(F, dtype=np.int64) * W


def frame_energy_ref(x, n: int, W: int, dt=np.float64):
    """-> (e, pk): per-frame mean power in `dt` (products and sum in dt, one division) and per-frame peak, vectorised."""
    n = int(n)
    F = (n + W - 1) // W
    pad = np.zeros(F * W, dt)
    pad[:n] = np.asarray(x[:n], dt)
    fr = pad.reshape(F, W)
    cnt = frame_counts(n, W)
    e = (np.sum(fr * fr, axis=1, dtype=dt) / cnt.astype(dt)).astype(dt) if F else np.zeros(0, dt)
    pk = np.abs(fr).max(axis=1).astype(np.float32) if F else np.zeros(0, np.float32)
    return e, pk


def frame_energy_naive(x, n: int, W: int, dt=np.float64):
    """The same, one sample at a time in ascending order."""
    n = int(n)
    F = (n + W - 1) // W
    e, pk = np.zeros(F, dt), np.zeros(F, np.float32)
    for f in range(F):
        s, m, c = dt(0), np.float32(0), 0
        for i in range(f * W, min(n, (f + 1) * W)):
            v = dt(x[i])
            s = dt(s + dt(v * v))
            m = max(m, np.float32(abs(np.float32(x[i]))))
            c += 1
        e[f] = dt(s / dt(c))
        pk[f] = m
    return e, pk


def speech_frames(e: np.ndarray, p) -> np.ndarray:
    """The local form of the speech test: active, and some window of min_run frames that contains f lies inside the row and is all
    active."""
    dt = e.dtype.type
    F = e.shape[0]
    if F == 0:
        return np.zeros(0, bool)
    thr = max(dt(dt(e.max()) * dt(p["rel_pow"])), dt(p["floor_pow"]))
    act = e > thr
    r = int(p["min_run"])
    c = np.concatenate([[0], np.cumsum(act)])
    full = np.zeros(F, bool)                      # full[s]: frames s .. s + r - 1 exist and are all active
    if F >= r:
        full[:F - r + 1] = (c[r:] - c[:F - r + 1]) == r
    sp = np.zeros(F, bool)
    for j in range(r):
        sp[j:] |= full[:F - j]
    return sp


def decide_ref(e: np.ndarray, pk: np.ndarray, n: int, p):
    """(start, n, gain) from per-frame energies (in e's dtype: fp32 = the kernel's operations, float64 = the reference) and peaks."""
    dt = e.dtype.type
    n, W = int(n), int(p["W"])
    sp = speech_frames(e, p)
    idx = np.nonzero(sp)[0]
    if idx.size == 0:
        return 0, 0, dt(1.0)
    start = max(0, int(idx[0]) * W - int(p["lead"]))
    stop = min(n, (int(idx[-1]) + 1) * W + int(p["tail"]))
    g = dt(1.0)
    if float(p["target_rms"]) != 0.0:
        cnt = frame_counts(n, W)
        P = dt(np.sum((e[sp] * cnt[sp].astype(dt)).astype(dt), dtype=dt) / dt(cnt[sp].sum()))
        g = dt(dt(p["target_rms"]) / dt(np.sqrt(P)))
        g = min(g, dt(p["max_gain"]))
        peak = dt(pk.max())
        if dt(peak * g) > dt(p["peak_limit"]):
            g = dt(dt(p["peak_limit"]) / peak)
    return start, stop - start, g


def decide_naive(e: np.ndarray, pk: np.ndarray, n: int, p):
    """The same from the wording: maximal runs of active frames found by a sequential scan, sums in ascending order."""
    dt = e.dtype.type
    n, W, F = int(n), int(p["W"]), e.shape[0]
    E = dt(0)
    for f in range(F):
        E = max(E, e[f])
    thr = max(dt(E * dt(p["rel_pow"])), dt(p["floor_pow"]))
    sp = [False] * F
    f = 0
    while f < F:
        if e[f] > thr:
            g = f
            while g < F and e[g] > thr:
                g += 1
            if g - f >= int(p["min_run"]):
                for k in range(f, g):
                    sp[k] = True
            f = g
        else:
            f += 1
    idx = [f for f in range(F) if sp[f]]
    if not idx:
        return 0, 0, dt(1.0)
    start = max(0, idx[0] * W - int(p["lead"]))
    stop = min(n, (idx[-1] + 1) * W + int(p["tail"]))
    g = dt(1.0)
    if float(p["target_rms"]) != 0.0:
        ps, cs, peak = dt(0), 0, dt(0)
        for f in idx:
            c = min(n, (f + 1) * W) - f * W
            ps = dt(ps + dt(e[f] * dt(c)))
            cs += c
        for f in range(F):
            peak = max(peak, dt(pk[f]))
        g = dt(dt(p["target_rms"]) / dt(np.sqrt(dt(ps / dt(cs)))))
        g = min(g, dt(p["max_gain"]))
        if dt(peak * g) > dt(p["peak_limit"]):
            g = dt(dt(p["peak_limit"]) / peak)
    return start, stop - start, g


def endpoints_ref(x, n: int, p, dt=np.float64):
    e, pk = frame_energy_ref(x, n, int(p["W"]), dt)
    return decide_ref(e, pk, n, p)


def margin_db(x, n: int, p) -> float:
    """Distance in dB of the float64 energy of the nearest non-zero frame from the row's threshold (inf for a row without one)."""
    e, _ = frame_energy_ref(x, n, int(p["W"]), np.float64)
    nz = e > 0
    if not nz.any():
        return float("inf")
    thr = max(e.max() * float(p["rel_pow"]), float(p["floor_pow"]))
    return float(np.min(np.abs(10 * np.log10(e[nz] / thr))))


ROW_KINDS = ("burst in silence", "burst over a noise floor", "burst and click in silence", "burst and click over a noise floor",
             "all zero", "all speech", "shorter than a frame", "empty")
CASE_SEEDS = tuple(range(20))
MIN_MARGIN_DB = 6.0


def endpoint_case(seed: int, p=None):
    """Eight crafted rows [(x fp32, n), ...], one of each ROW_KINDS: a noise burst somewhere in the row, in exact silence or over a
    noise floor 70 dB down, with or without a two-frame click in the leading silence (shorter than min_run = 3), an all-zero row, a
    row that is all speech, one shorter than a frame, an empty one.  Asserts (does not skip, drops nothing) that every frame with
    non-zero energy lies at least MIN_MARGIN_DB from its row's threshold in float64, so that fp32 and float64 cannot disagree
    about a decision."""
    p = p or DEFAULT_PARAMS
    W = int(p["W"])
    g = np.random.default_rng(seed)
    rows = []
    for kind in range(8):
        n = int(g.integers(1, 30)) * 3200 if kind != 6 else int(g.integers(1, W))
        if kind == 7:
            n = 0
        x = np.zeros(max(n, 1), np.float32)
        if kind in (0, 1, 2, 3) and n:
            a = int(g.integers(W * 8, n // 2)) if n // 2 > W * 8 else 0
            b = int(g.integers(n // 2, n))
            amp = 10 ** g.uniform(-1.5, -0.3)
            x[a:b] = (g.standard_normal(b - a) * amp).astype(np.float32)
            if kind in (1, 3):
                x[:n] += (g.standard_normal(n) * amp * 10 ** (-70 / 20)).astype(np.float32)
            if kind in (2, 3) and a > W * 6:
                c = W * 2
                x[c:c + 2 * W] += (g.standard_normal(2 * W) * amp).astype(np.float32)
        if kind == 5 and n:
            x[:n] = (g.standard_normal(n) * 0.2).astype(np.float32)
        if kind == 6 and n:
            x[:n] = 0.3
        m = margin_db(x, n, p)
        assert m >= MIN_MARGIN_DB, f"seed {seed} row {kind} ({ROW_KINDS[kind]}): a frame lies {m:.2f} dB from the threshold"
        rows.append((x, n))
    return rows


def pad_batch(rows, fill=np.nan, stride=None):
    """rows [(x, n)] -> (audio (B,1,S) fp32 with `fill` behind every row's n samples, lens): a read past a row shows."""
    S = stride or max(max(n for _, n in rows), 1)
    audio = np.full((len(rows), 1, S), fill, np.float32)
    for b, (x, n) in enumerate(rows):
        audio[b, 0, :n] = x[:n]
    return audio, [n for _, n in rows]


def stitch_seg_numpy(out: np.ndarray, audio: np.ndarray, seg, gain, offsets, fade: np.ndarray) -> np.ndarray:
    """Windows audio[b, 0, start : start + n] times gain[b] (gain None: no multiply), then faded by the table over the window's own
    ends (F_b = min(F, n // 2)), into out (1-D fp32 or int16) at offsets[b]; every step one fp32 multiply.  Vectorised per row."""
    fade = np.asarray(fade, np.float32)
    F = fade.shape[0]
    for b, o in enumerate(offsets):
        s, n, o = int(seg[b][0]), int(seg[b][1]), int(o)
        row = np.array(audio[b, 0, s:s + n], np.float32)
        if gain is not None:
            row = row * np.float32(gain[b])
        Fb = min(F, n // 2)
        if Fb:
            row[:Fb] = row[:Fb] * fade[:Fb]
            row[n - Fb:] = row[n - Fb:] * fade[:Fb][::-1]
        out[o:o + n] = pcm16_numpy(row) if out.dtype == np.int16 else row
    return out


def stitch_seg_naive(out: np.ndarray, audio: np.ndarray, seg, gain, offsets, fade: np.ndarray) -> np.ndarray:
    """The same definition, one sample at a time."""
    F = len(fade)
    for b in range(len(offsets)):
        s, n = int(seg[b][0]), int(seg[b][1])
        Fb = min(F, n // 2)
        for i in range(n):
            v = np.float32(audio[b, 0, s + i])
            if gain is not None:
                v = np.float32(v * np.float32(gain[b]))
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
