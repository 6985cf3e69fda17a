"""python tools/long_stream_bench.py --variant long|stream|profile [--tree DIR] [--pieces 40] [--reps 15] [--warmup 3] [--precision f16] [--out FILE.json]
What handing a long text out early buys and costs: default precision, full-size codec, seeded synthetic weights, one voice
of 15 reference frames, `--pieces` pieces of 40 .. 75 frames (5.3 .. 10 s) and 30 tokens each, max_batch 8, three groups in flight.
Each variant in a process of its own:
* long:    synthesize_long of the text as it always was.  `--tree DIR` imports smalltts_amd from another checkout (built there), so
  the same figure can be taken on the parent commit: that path is unchanged and the two must agree within the spread that two
  processes of one tree show;
* stream:  synthesize_long, synthesize_long_stream with the default ramp (1, 2, 4, 8) and with batch_sizes=None, alternating call by
  call: wall time from the call to its first chunk and to its last;
* profile: the library's per-kernel profiler over engine.join_stream alone on 8 x 10 s of audio, fp32 and PCM16: time per launch of
  the main kernel and of the state launch.
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
    ap.add_argument("--variant", required=True, choices=["long", "stream", "profile"])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout to import smalltts_amd from")
    ap.add_argument("--pieces", type=int, default=40)
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
    voice = tts.encode_voice(g.standard_normal((15, 64)).astype(np.float32))
    toks = [[int(t) for t in g.integers(1, 198, size=30)] for _ in range(args.pieces)]
    durs = [float(f) / 7.5 + 0.01 for f in g.integers(40, 76, size=args.pieces)]
    kw = dict(token_lists=toks, durations=durs, seed=5, max_batch=8, in_flight=3)
    out = {"variant": args.variant, "precision": args.precision, "pieces": args.pieces, "tree": os.path.abspath(args.tree)}

    def whole():
        tts.synthesize_long(voice, **kw)

    def stream(batch_sizes):
        t0, first = time.perf_counter(), None
        for _c in tts.synthesize_long_stream(voice, batch_sizes=batch_sizes, **kw):
            first = (time.perf_counter() - t0) * 1e3 if first is None else first
        return first

    if args.variant == "profile":
        B, n = 8, 75
        audio = (0.3 * torch.randn(B, 1, eng.hop * n, generator=torch.Generator().manual_seed(3))).to(eng.device)
        seg = torch.tensor([[0, eng.hop * n]] * B, dtype=torch.int64, device=eng.device)
        fade = torch.from_numpy(np.linspace(0.0, 1.0, 120, dtype=np.float32)).to(eng.device)
        out["kernels"] = {}
        for pcm16 in (False, True):
            state = eng.join_state()
            run = lambda: eng.join_stream(audio, seg, None, fade, 2880, state, last=False, pcm16=pcm16)
            for _ in range(args.warmup):
                run()
            torch.cuda.synchronize()
            eng.profile(True)
            for _ in range(args.reps):
                run()
            torch.cuda.synchronize()
            rep = eng.profile_report()
            eng.profile(False)
            name = "8 x 10 s " + ("pcm16" if pcm16 else "f32")
            out["kernels"][name] = {e["name"]: {"us_per_launch": round(1e3 * e["ms"] / max(e["launches"], 1), 3),
                                                "launches_per_call": e["launches"] // args.reps} for e in rep if "join" in e["name"]}
            print(f"[join kernels, {name}] {out['kernels'][name]}")
    else:
        shapes = {"synthesize_long": whole}
        if args.variant == "stream":
            shapes["stream (1, 2, 4, 8)"] = lambda: stream((1, 2, 4, 8))
            shapes["stream None"] = lambda: stream(None)
        for call in shapes.values():
            for _ in range(args.warmup):
                call()
        total = {s: [] for s in shapes}
        first = {s: [] for s in shapes}
        for _ in range(args.reps):
            for s, call in shapes.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f = call()
                total[s].append((time.perf_counter() - t0) * 1e3)
                if f is not None:
                    first[s].append(f)
        out["ms"] = {}
        for s in shapes:
            out["ms"][s] = {"total": stats(total[s])}
            line = f"[{args.variant}, {args.pieces} pieces, {args.reps} calls] {s}: total median {statistics.median(total[s]):.2f} ms ({min(total[s]):.2f} - {max(total[s]):.2f})"
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
