"""python tools/pitch_bench.py [--reps 10] [--out FILE.json]
The time of smtts_pitch's two kernels for B = 8 rows of 10 s at the defaults of options.Pitch (NOTEBOOK "Pitch"), by the
library's own per-kernel profiler (HIP events around every launch), on three inputs: the audio a synthesize_batch of 8 x 10 s returns
(full-size synthetic weights, default precision), four-harmonic tones, and white noise; and next to it the wall time of that
synthesize_batch (its third call) and of a pitch call, both ending in a device synchronise.  Per call and per frame (8 x 1000)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, SECONDS, SEED = 8, 10, 20260928


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from smalltts_amd.api import SmallTTS
    from smalltts_amd.engine import HipEngine
    from smalltts_amd.options import Pitch
    eng = HipEngine(0)
    eng.load_synthetic(SEED, parts=("dit", "decoder", "encoder"))
    eng.finalize()
    tts = SmallTTS(engine=eng, seed=0)
    g = torch.Generator().manual_seed(1)
    refs = [torch.randn(15, 64, generator=g).numpy() for _ in range(B)]
    toks = [[1 + i % 197 for i in range(40)]] * B
    synth_ms = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        audio = tts.synthesize_batch(refs, toks, [float(SECONDS)] * B)
        torch.cuda.synchronize()
        synth_ms.append(round(1e3 * (time.perf_counter() - t0), 2))
    n = SECONDS * 24000
    t = np.arange(n) / 24000.0
    tone = np.stack([sum(np.sin(2 * np.pi * (k + 1) * f0 * t) / (k + 1) for k in range(4)) * 0.25 for f0 in np.linspace(80, 320, B)])
    inputs = {"synthesized": np.stack([np.asarray(a, np.float32).reshape(-1)[:n] for a in audio]),
              "tones": tone.astype(np.float32), "noise": (0.1 * np.random.default_rng(0).standard_normal((B, n))).astype(np.float32)}
    pt = Pitch()
    frames = B * (-(-n // pt.hop))
    out = {"rows": B, "seconds": SECONDS, "reps": args.reps, "frames_per_call": frames, "synthesize_batch_ms": synth_ms, "inputs": {}}
    for name, x in inputs.items():
        y = torch.from_numpy(np.ascontiguousarray(x)).to(eng.device).view(B, 1, n)
        for _ in range(3):
            lag, _peak = eng.pitch(y, [n] * B, pt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            eng.pitch(y, [n] * B, pt)
        torch.cuda.synchronize()
        wall = 1e3 * (time.perf_counter() - t0) / args.reps
        eng.profile(True)
        for _ in range(args.reps):
            eng.pitch(y, [n] * B, pt)
        torch.cuda.synchronize()
        report = eng.profile_report()
        eng.profile(False)
        row = {"wall_ms_per_call": round(wall, 3), "voiced_share": round(float((lag > 0).float().mean()), 3)}
        for e in report:
            if e["name"] in ("pitch_score", "pitch_path"):
                ms = e["ms"] / max(e["launches"], 1)
                row[e["name"]] = {"ms_per_call": round(ms, 3), "us_per_frame": round(1e3 * ms / frames, 4), "launches": e["launches"]}
                print(f"[{name}, {B} rows x {SECONDS} s] {e['name']}: {ms:.3f} ms per call, {1e3 * ms / frames:.3f} us per frame "
                      f"({e['launches']} launches)")
        print(f"[{name}] wall {wall:.3f} ms per call, voiced share {row['voiced_share']}; synthesize_batch {synth_ms} ms")
        out["inputs"][name] = row
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
