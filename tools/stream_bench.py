"""python tools/stream_bench.py --variant stream|whole|profile [--reps 15] [--warmup 3] [--precision f16] [--out FILE.json]
What streaming the codec buys and costs, under latency tuning, at 1 x 10 s, 1 x 30 s and 8 x 30 s (75 / 225 frames,
reference 15 frames, 30 tokens, 4 DMD steps, the full-size codec, seeded synthetic weights).  Each variant in a process of its own:
* stream: wall time from the call of synthesize_stream to its first yielded chunk and to its last one (8 x 30 s: eight calls one
  after the other, as a caller that speaks one utterance at a time makes them; the first chunk is that of the first call);
* whole:  wall time of synthesize (8 x 30 s: synthesize_batch of the eight rows) — run it on the parent commit as well for the
  figure streaming is compared against;
* profile: the library's per-kernel profiler over the codec alone: codec_decode of (B, N) against the same frames through
  codec_decode_stream in synthesize_stream's chunks, total device time of either, and carry_frames' time per launch.
`--warmup` calls of every shape first, then the shapes alternate call by call; median (min - max) of `--reps` calls."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"1 x 10 s": (1, 75), "1 x 30 s": (1, 225), "8 x 30 s": (8, 225)}


def stats(t):
    return {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", required=True, choices=["stream", "whole", "profile"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from smalltts_amd.api import SmallTTS
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0, args.precision)
    eng.load_synthetic(7, parts=("dit", "decoder", "encoder"))
    eng.finalize()
    eng.set_tuning("latency")
    tts = SmallTTS(engine=eng, seed=1)
    g = np.random.default_rng(0)
    ref = g.standard_normal((15, 64)).astype(np.float32)
    toks = [[int(t) for t in g.integers(1, 198, size=30)] for _ in range(8)]
    out = {"variant": args.variant, "precision": args.precision, "tuning": "latency"}

    def whole(B, n):
        tts.synthesize_batch([ref] * B, toks[:B], None, frames=[n] * B, seeds=list(range(50, 50 + B)))
        return None

    def stream(B, n):
        t0, first = time.perf_counter(), None
        for b in range(B):
            for _c in tts.synthesize_stream(ref, toks[b], None, frames=n, seed=50 + b):
                first = (time.perf_counter() - t0) * 1e3 if first is None else first
        return first

    if args.variant == "profile":
        from smalltts_amd.api import stream_chunks
        out["codec"] = {}
        for name, (B, n) in SHAPES.items():
            lat = torch.randn(B, n, 64, generator=torch.Generator().manual_seed(3)).to(eng.device)
            res = {}
            for kind in ("whole", "chunked"):
                def run():
                    if kind == "whole":
                        eng.codec_decode(lat)
                    else:
                        state, t0 = eng.decode_state(B), 0
                        for c in stream_chunks(n):
                            eng.codec_decode_stream(lat[:, t0:t0 + c], state, list(range(B)))
                            t0 += c
                for _ in range(args.warmup):
                    run()
                torch.cuda.synchronize()
                eng.profile(True)
                for _ in range(args.reps):
                    run()
                torch.cuda.synchronize()
                rep = eng.profile_report()
                eng.profile(False)
                res[kind + "_ms_per_call"] = round(sum(e["ms"] for e in rep) / args.reps, 4)
                res[kind + "_launches_per_call"] = sum(e["launches"] for e in rep) // args.reps
                for e in rep:
                    if "carry_frames" in e["name"]:
                        res["carry_frames_us_per_launch"] = round(1e3 * e["ms"] / max(e["launches"], 1), 3)
                        res["carry_frames_launches_per_call"] = e["launches"] // args.reps
            out["codec"][name] = res
            print(f"[codec kernels, {name}] {res}")
    else:
        call = whole if args.variant == "whole" else stream
        for B, n in SHAPES.values():
            for _ in range(args.warmup):
                call(B, n)
        total = {s: [] for s in SHAPES}
        first = {s: [] for s in SHAPES}
        for _ in range(args.reps):
            for s, (B, n) in SHAPES.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f = call(B, n)
                total[s].append((time.perf_counter() - t0) * 1e3)
                if f is not None:
                    first[s].append(f)
        out["ms"] = {}
        for s in SHAPES:
            out["ms"][s] = {"total": stats(total[s])}
            line = f"[{args.variant}, {args.reps} calls] {s}: total median {statistics.median(total[s]):.2f} ms ({min(total[s]):.2f} - {max(total[s]):.2f})"
            if first[s]:
                out["ms"][s]["first_chunk"] = stats(first[s])
                line += f"; first chunk median {statistics.median(first[s]):.2f} ms ({min(first[s]):.2f} - {max(first[s]):.2f})"
            print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
