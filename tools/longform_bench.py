#!/usr/bin/env python
"""Long-form synthesis against what the package offered before it, on one GPU, in one process.

A 24-piece paragraph in one voice (full-size codec, seeded synthetic weights, the default precision), timed
  (a) through SmallTTS.synthesize_long: the voice encoded once, per-row noise in one launch per batch, rows joined on the device,
      one device-to-host copy;
  (b) through SmallTTS.synthesize_batches with the reference latents repeated for every row (the style encoder runs per row and
      batch), one device-to-host copy per batch and the fade / gap / join in numpy on the host;
same batches of 8, same in_flight, same (throughput) tuning.  Both legs are warmed up on the shapes they time, then alternate
a, b, a, b ... so that drift of the shared host hits both alike; every repetition ends in a host copy of the audio, so the host
clock brackets finished device work.  Prints one JSON line: medians, min / max and the run-to-run spread of each leg.

--trim times another pair instead, the same way: (a) as above against (t) synthesize_long(trim=True), the endpoint kernels behind
every batch's decode, one small read-back, the join over the speech windows; "trim_over_plain" is the ratio of their medians.

    python tools/longform_bench.py [--reps 15] [--warmup 3] [--in-flight 3] [--weights synthetic:7] [--trim]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECES, MAX_BATCH, REF_FRAMES = 24, 8, 38     # 38 reference frames = a 5 s clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--in-flight", type=int, default=3)
    ap.add_argument("--weights", default="synthetic:7")
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--trim", action="store_true", help="time synthesize_long with and without trim=True instead of legs (a) / (b)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("longform_bench: needs a GPU (a CPU run measures nothing about it)")
    from smalltts_amd.api import HOP_SIZE, SmallTTS, fade_table, plan_long

    tts = SmallTTS(weights=args.weights, precision=args.precision, seed=0)
    g = np.random.default_rng(2)
    ref = g.standard_normal((REF_FRAMES, 64)).astype(np.float32)
    durs = [float(d) for d in g.uniform(4.0, 14.0, size=PIECES)]              # sentences of 4 - 14 s: 30 - 105 frames
    toks = [[int(t) for t in g.integers(1, 198, size=int(12 * d))] for d in durs]   # ~12 phonemes per second
    ns = [max(1, int(d * 7.5)) for d in durs]
    groups, offsets, S = plan_long(ns, MAX_BATCH, 120.0)
    fade = fade_table(5.0)

    def leg_a():
        voice = tts.encode_voice(ref)     # part of the cost of a call: once per paragraph
        return tts.synthesize_long(voice, token_lists=toks, durations=durs, seed=3, max_batch=MAX_BATCH, in_flight=args.in_flight)

    def leg_b():
        batches = [([ref] * len(gr), [toks[i] for i in gr], [durs[i] for i in gr]) for gr in groups]
        outs = tts.synthesize_batches(batches, in_flight=args.in_flight)
        y = np.zeros((1, S), np.float32)
        F = len(fade)
        for gr, rows in zip(groups, outs):
            for i, row in zip(gr, rows):
                r = row[0].copy()
                Fb = min(F, r.size // 2)
                if Fb:
                    r[:Fb] *= fade[:Fb]
                    r[-Fb:] *= fade[:Fb][::-1]
                y[0, offsets[i]:offsets[i] + r.size] = r
        return y

    def leg_t():
        voice = tts.encode_voice(ref)
        return tts.synthesize_long(voice, token_lists=toks, durations=durs, seed=3, max_batch=MAX_BATCH, in_flight=args.in_flight, trim=True)

    other = leg_t if args.trim else leg_b
    for _ in range(args.warmup):
        a, b = leg_a(), other()
    assert a.shape == (1, S) and np.isfinite(a).all() and np.isfinite(b).all() and (b.shape == a.shape or args.trim)
    ta, tb = [], []
    for _ in range(args.reps):
        for fn, acc in ((leg_a, ta), (other, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            acc.append((time.perf_counter() - t0) * 1e3)

    def stats(t):
        t = np.asarray(t)
        return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3), "max_ms": round(float(t.max()), 3),
                "spread": round(float((t.max() - t.min()) / np.median(t)), 4)}

    audio_s = sum(HOP_SIZE * n for n in ns) / 24000.0
    if args.trim:
        print(json.dumps({"tool": "longform_bench --trim", "pieces": PIECES, "max_batch": MAX_BATCH, "in_flight": args.in_flight,
                          "audio_seconds": round(audio_s, 2), "trimmed_seconds": round(b.shape[1] / 24000.0, 2), "reps": args.reps,
                          "warmup": args.warmup, "precision": args.precision, "synthesize_long": stats(ta),
                          "synthesize_long_trim": stats(tb), "trim_over_plain": round(float(np.median(tb) / np.median(ta)), 4)}))
        return
    print(json.dumps({"tool": "longform_bench", "pieces": PIECES, "max_batch": MAX_BATCH, "in_flight": args.in_flight, "ref_frames": REF_FRAMES,
                      "audio_seconds": round(audio_s, 2), "reps": args.reps, "warmup": args.warmup, "precision": args.precision,
                      "synthesize_long": stats(ta), "synthesize_batches_host_join": stats(tb),
                      "long_over_batches": round(float(np.median(ta) / np.median(tb)), 4)}))


if __name__ == "__main__":
    main()
