"""python tools/deliver_bench.py --variant batch|plain|stream|profile [--tree DIR] [--reps 15] [--warmup 3] [--precision f16] [--out FILE.json]
What delivery at the caller's rate and encoding costs, under latency tuning, full-size codec, seeded synthetic weights,
reference 15 frames, 30 tokens, 4 DMD steps.  Each variant in a process of its own:
* plain:   synthesize_batch of 8 x 10 s (75 frames) as it always was.  `--tree DIR` imports smalltts_amd from another checkout (built
  there), so the same figure can be taken on the parent commit: the plain path is unchanged and the two must agree within the spread;
* batch:   the same call plain, with Delivery(8000, "mulaw") and with Delivery(48000, "pcm16"), alternating call by call;
* stream:  synthesize_stream of 1 x 10 s, plain and with Delivery(8000, "mulaw"), alternating: wall time from the call to its first
  and to its last yielded chunk;
* profile: the library's per-kernel profiler over engine.deliver alone on 8 x 10 s of audio: time per launch of the main kernel and
  of the history launch at every rate (mu-law; whole and streamed in synthesize_stream's chunks at 8 kHz).
`--warmup` calls of every shape first, then the shapes alternate call by call; median (min - max) of `--reps` calls."""
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
    ap.add_argument("--variant", required=True, choices=["plain", "batch", "stream", "profile"])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import smalltts_amd from")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
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
    B, n = 8, 75
    out = {"variant": args.variant, "precision": args.precision, "tuning": "latency", "tree": os.path.abspath(args.tree)}

    def batch(dv):
        kw = {} if dv is None else {"deliver": dv}
        tts.synthesize_batch([ref] * B, toks, None, frames=[n] * B, seeds=list(range(50, 50 + B)), **kw)

    def stream(dv):
        kw = {} if dv is None else {"deliver": dv}
        t0, first = time.perf_counter(), None
        for _c in tts.synthesize_stream(ref, toks[0], None, frames=n, seed=50, **kw):
            first = (time.perf_counter() - t0) * 1e3 if first is None else first
        return first

    if args.variant == "profile":
        from smalltts_amd.api import stream_chunks
        from smalltts_amd.audio import DELIVER_RATES
        audio = (0.3 * torch.randn(B, 1, eng.hop * n, generator=torch.Generator().manual_seed(3))).to(eng.device)
        out["kernels"] = {}

        def timed(run):
            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            eng.profile(True)
            for _ in range(args.reps):
                run()
            torch.cuda.synchronize()
            rep = eng.profile_report()
            eng.profile(False)
            return {e["name"]: {"us_per_launch": round(1e3 * e["ms"] / max(e["launches"], 1), 3), "launches_per_call": e["launches"] // args.reps}
                    for e in rep if "deliver" in e["name"]}

        for rate in DELIVER_RATES:
            out["kernels"][f"{rate} whole"] = timed(lambda: eng.deliver(audio, [eng.hop * n] * B, rate, "mulaw"))
            print(f"[deliver kernels, 8 x 10 s, {rate} Hz mu-law, whole] {out['kernels'][f'{rate} whole']}")

        def chunked():
            state, t0 = eng.deliver_state(B, 8000), 0
            sizes = stream_chunks(n)
            for k, c in enumerate(sizes):
                a = audio[:, :, eng.hop * t0: eng.hop * (t0 + c)].contiguous()
                eng.deliver(a, [eng.hop * c] * B, 8000, "mulaw", state=state, slots=list(range(B)), n_before=[eng.hop * t0] * B,
                            last=k == len(sizes) - 1)
                t0 += c
        out["kernels"]["8000 chunked"] = timed(chunked)
        print(f"[deliver kernels, 8 x 10 s, 8000 Hz mu-law, in synthesize_stream's chunks] {out['kernels']['8000 chunked']}")
    else:
        if args.variant == "plain":
            shapes = {"8 x 10 s plain": (batch, None)}
        else:
            from smalltts_amd.api import Delivery
            call = batch if args.variant == "batch" else stream
            name = "8 x 10 s" if args.variant == "batch" else "1 x 10 s stream"
            shapes = {f"{name} plain": (call, None), f"{name} 8 kHz mu-law": (call, Delivery(8000, "mulaw"))}
            if args.variant == "batch":
                shapes[f"{name} 48 kHz pcm16"] = (call, Delivery(48000, "pcm16"))
        for call, dv in shapes.values():
            for _ in range(args.warmup):
                call(dv)
        total = {s: [] for s in shapes}
        first = {s: [] for s in shapes}
        for _ in range(args.reps):
            for s, (call, dv) in shapes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f = call(dv)
                total[s].append((time.perf_counter() - t0) * 1e3)
                if f is not None:
                    first[s].append(f)
        out["ms"] = {}
        for s in shapes:
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
