"""python tools/watermark_bench.py --variant profile|long [--pieces 40] [--reps 15] [--warmup 3] [--precision f16] [--out FILE.json]
What the watermark costs, by the method of tools/long_stream_bench.py: default precision, full-size codec, seeded
synthetic weights.  Each variant in a process of its own:
* profile: the library's per-kernel profiler over engine.watermark on 8 x 10 s of audio (with a pool: the main and the carry launch)
  and over engine.watermark_detect on 10 s with 65 536 offsets (its three launches): time per launch;
* long:    synthesize_long of long_stream_bench's text without and with watermark=, alternating call by call: wall time per call.
  The un-marked path against the parent commit: tools/long_stream_bench.py --variant long [--tree PARENT].
`--warmup` calls of every shape first; median (min - max) of `--reps` calls."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def stats(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", required=True, choices=["profile", "long"])
    ap.add_argument("--pieces", type=int, default=40)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from smalltts_amd.api import SmallTTS, Watermark
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0, args.precision)
    out = {"variant": args.variant, "precision": args.precision}
    key = 0x5EEDC0DE12345678

    def kernels(run, what):
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        eng.profile(True)
        for _ in range(args.reps):
            run()
        torch.cuda.synchronize()
        rep = eng.profile_report()
        eng.profile(False)
        res = {e["name"]: {"us_per_launch": round(1e3 * e["ms"] / max(e["launches"], 1), 3), "launches_per_call": e["launches"] // args.reps}
               for e in rep if "watermark" in e["name"]}
        print(f"[watermark kernels, {what}] {res}")
        return res

    if args.variant == "profile":
        B, n = 8, 240_000
        audio = (0.3 * torch.randn(B, 1, n, generator=torch.Generator().manual_seed(3))).to(eng.device)
        state = eng.watermark_state(B)
        out["kernels"] = {
            "embed 8 x 10 s": kernels(lambda: eng.watermark(audio, [n] * B, key, 0.02, state=state, slots=list(range(B)), n_before=[0] * B),
                                      "embed 8 x 10 s"),
            "detect 10 s x 65536 offsets": kernels(lambda: eng.watermark_detect(audio[0], [n], key, o_lo=0, n_off=65536),
                                                   "detect 10 s x 65536 offsets"),
            "detect 10 s x 1 offset": kernels(lambda: eng.watermark_detect(audio[0], [n], key, o_lo=0, n_off=1), "detect 10 s x 1 offset"),
        }
    else:
        eng.load_synthetic(7, parts=("dit", "decoder", "encoder"))
        eng.finalize()
        eng.set_tuning("latency")
        tts = SmallTTS(engine=eng, seed=1)
        g = np.random.default_rng(0)
        voice = tts.encode_voice(g.standard_normal((15, 64)).astype(np.float32))
        toks = [[int(t) for t in g.integers(1, 198, size=30)] for _ in range(args.pieces)]
        durs = [float(f) / 7.5 + 0.01 for f in g.integers(40, 76, size=args.pieces)]
        kw = dict(token_lists=toks, durations=durs, seed=5, max_batch=8, in_flight=3)
        shapes = {"synthesize_long": lambda: tts.synthesize_long(voice, **kw),
                  "synthesize_long watermark=": lambda: tts.synthesize_long(voice, watermark=Watermark(key), **kw)}
        for call in shapes.values():
            for _ in range(args.warmup):
                call()
        total = {s: [] for s in shapes}
        for _ in range(args.reps):
            for s, call in shapes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                total[s].append((time.perf_counter() - t0) * 1e3)
        out["pieces"] = args.pieces
        out["ms"] = {s: stats(total[s]) for s in shapes}
        for s in shapes:
            print(f"[long, {args.pieces} pieces, {args.reps} calls] {s}: median {statistics.median(total[s]):.2f} ms ({min(total[s]):.2f} - {max(total[s]):.2f})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
