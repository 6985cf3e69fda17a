#!/usr/bin/env python
"""What word timings cost, on one GPU, in one process.

Full-size codec, seeded synthetic weights, the default precision.  Three measurements:
  batch   synthesize_batch at the bench shape (8 rows x 10 s, 15 reference frames, 30 tokens) with alignment off and on;
  long    synthesize_long over the 24-piece paragraph of tools/longform_bench.py with return_words off and on;
  kernels the time per launch of the two new kernels (attn_text_mass: 12 launches per sampler call at the default selection; align_path:
          one), from the engine's per-kernel HIP-event profile of one aligned batch at the bench shape.
Both legs of a pair are warmed up on the shapes they time, then alternate off, on, off, on ... so that drift of the shared host hits
both alike; every repetition ends in a host copy, so the host clock brackets finished device work.  Prints one JSON line: medians,
min / max, the run-to-run spread of each leg and on / off.

    python tools/align_bench.py [--reps 15] [--warmup 3] [--in-flight 3] [--weights synthetic:7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIECES, MAX_BATCH, REF_FRAMES = 24, 8, 38     # the paragraph of tools/longform_bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--in-flight", type=int, default=3)
    ap.add_argument("--weights", default="synthetic:7")
    ap.add_argument("--precision", default="f16")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("align_bench: needs a GPU (a CPU run measures nothing about it)")
    from smalltts_amd.api import HOP_SIZE, SmallTTS

    tts = SmallTTS(weights=args.weights, precision=args.precision, seed=0)
    eng = tts.engine
    g = np.random.default_rng(2)
    ref = g.standard_normal((REF_FRAMES, 64)).astype(np.float32)
    durs = [float(d) for d in g.uniform(4.0, 14.0, size=PIECES)]
    toks = [[int(t) for t in g.integers(1, 198, size=int(12 * d))] for d in durs]
    b_refs = [g.standard_normal((15, 64)).astype(np.float32) for _ in range(8)]
    b_toks = [[int(t) for t in g.integers(1, 198, size=30)] for _ in range(8)]
    b_noise = torch.randn(4, 8, 75, 64, generator=torch.Generator().manual_seed(1))

    def batch(on):
        return tts.synthesize_batch(b_refs, b_toks, 10.0, noise=b_noise, **({"align": True} if on else {}))

    def long(on):
        voice = tts.encode_voice(ref)     # part of the cost of a call: once per paragraph
        return tts.synthesize_long(voice, token_lists=toks, durations=durs, seed=3, max_batch=MAX_BATCH, in_flight=args.in_flight,
                                   return_words=on)

    def stats(t):
        t = np.asarray(t)
        return {"median_ms": round(float(np.median(t)), 3), "min_ms": round(float(t.min()), 3), "max_ms": round(float(t.max()), 3),
                "spread": round(float((t.max() - t.min()) / np.median(t)), 4)}

    def pair(fn):
        for _ in range(args.warmup):
            off, on = fn(False), fn(True)
        t_off, t_on = [], []
        for _ in range(args.reps):
            for flag, acc in ((False, t_off), (True, t_on)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(flag)
                acc.append((time.perf_counter() - t0) * 1e3)
        return off, on, {"off": stats(t_off), "on": stats(t_on), "on_over_off": round(float(np.median(t_on) / np.median(t_off)), 4)}

    off, on, r_batch = pair(batch)
    assert all(np.array_equal(a, b) for a, b in zip(off, on[0])), "alignment moved the audio"
    r_batch["word_groups"] = sum(len(w) for w in on[1])
    off, on, r_long = pair(long)
    assert np.array_equal(off, on[0]), "alignment moved the audio"
    r_long["word_groups"] = len(on[1])
    r_long["audio_seconds"] = round(sum(HOP_SIZE * max(1, int(d * 7.5)) for d in durs) / 24000.0, 2)

    # per-launch time of the new kernels: one aligned batch under the per-kernel profile (latency tuning, one call at a time)
    eng.profile(True)
    for _ in range(3):
        batch(True)
    torch.cuda.synchronize()
    rep = {r["name"]: r for r in eng.profile_report()}
    eng.profile(False)
    kernels = {}
    for name in ("attn_text_mass", "align_path", "attention_img<128>"):
        r = rep.get(name)
        if r:
            kernels[name] = {"launches": r["launches"], "us_per_launch": round(1e3 * r["ms"] / r["launches"], 2),
                             "gflop_per_launch": round(r["flops"] / r["launches"] / 1e9, 4)}
    kernels["all_kernels_ms_per_call"] = round(sum(r["ms"] for r in rep.values()) / 3, 3)
    print(json.dumps({"tool": "align_bench", "reps": args.reps, "warmup": args.warmup, "in_flight": args.in_flight, "precision": args.precision,
                      "synthesize_batch_8x10s": r_batch, "synthesize_long_24_pieces": r_long, "kernels": kernels}))


if __name__ == "__main__":
    main()
