"""python tools/pinned_bench.py [--reps 30] [--warmup 5] [--precision f16]
What the select of pinned sampling costs: eng.sample at the benchmark shape (8 x 75 frames, R 15, P 30, 4 DMD steps), both tunings,
three variants on one build: plain (axpby), every frame free (x_pin given, nothing pinned), half the frames pinned.  Median (min - max)
of `--reps` calls after `--warmup`, each timed with a pair of HIP events on the sampler's stream; the variants alternate call by call so
that drift hits them alike.  Seeded synthetic weights (NOTEBOOK "Pinned sampling")."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="f16")
    args = ap.parse_args(argv)
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0, args.precision)
    eng.load_synthetic(7, parts=("dit",))
    eng.finalize()
    B, N, R, P = 8, 75, 15, 30
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(B, R, 64, generator=g)
    ids = torch.arange(1, P + 1)[None].repeat(B, 1)
    mask = torch.ones(B, N, dtype=torch.bool, device=eng.device)
    noise = torch.randn(4, B, N, 64, generator=g).to(eng.device)
    x_pin = torch.randn(B, N, 64, generator=g).to(eng.device)
    half = torch.zeros(B, N, dtype=torch.bool, device=eng.device)
    half[:, ::2] = True
    cache = eng.cond_encode(ref, torch.full((B,), R), ids, torch.ones(B, P, dtype=torch.bool))
    variants = {"plain": {}, "all free": dict(x_pin=x_pin), "half pinned": dict(x_pin=x_pin, pin=half)}
    out = {}
    for tuning in ("latency", "throughput"):
        prev = eng.set_tuning(tuning)
        try:
            ms = {k: [] for k in variants}
            for rep in range(args.warmup + args.reps):
                for name, kw in variants.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    eng.sample(cache, mask, num_steps=4, noise=noise, **kw)
                    b.record()
                    b.synchronize()
                    if rep >= args.warmup:
                        ms[name].append(a.elapsed_time(b))
        finally:
            eng.set_tuning(prev)
        for name, v in ms.items():
            out[f"{tuning} / {name}"] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4), n=len(v))
            print(f"{tuning:10s} {name:12s} median {np.median(v):.3f} ms  ({min(v):.3f} - {max(v):.3f}, n = {len(v)})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
