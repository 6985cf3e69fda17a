"""python tools/repair_bench.py --only profile|wall [--reps 15] [--warmup 3] [--profile-reps 20] [--precision f16] [--out FILE.json]
What repair costs at the benchmark shape (8 pieces x 75 frames, reference 15 frames, 30 tokens, 4 DMD steps, the full-size codec,
seeded synthetic weights), two measurements, each in a run of its own (the profiler's events slow the host, so the wall times are
taken in a process that never switched it on):
* the library's own per-kernel profiler (HIP events around every launch) over `--profile-reps` calls of
  synthesize_batch(repair=1) on the 8 rows, one call at a time; the lines of repair_plan, repair_keep, take_scores, align_path and
  the tap are printed;
* the wall time of synthesize_long on the same eight pieces without repair, with repair = 1, with takes = 2 and with takes = 2,
  repair = 1: a host clock around the call, which ends in the copy of the waveform to the host (a synchronise); `--warmup` calls of
  every variant first, then the variants alternate call by call so that drift hits them alike; median (min - max) of `--reps` calls.
  `--plain-only` times the call without repair alone: the figure to take on the parent commit, where the others do not exist."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("repair_plan", "repair_keep", "take_scores", "take_select", "align_path", "attn_text_mass")


def kernel_lines(report):
    """The entries of a profile report (a list of {name, launches, ms, ...}) that name one of KERNELS, with the time per launch."""
    return {e["name"]: dict(e, us_per_launch=round(1e3 * e["ms"] / max(e["launches"], 1), 3)) for e in report
            if any(k in e["name"] for k in KERNELS)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", required=True, choices=["profile", "wall"], help="which of the two measurements this run takes")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-reps", type=int, default=20)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--plain-only", action="store_true", help="wall: time the call without repair alone (runs on a commit without repair)")
    ap.add_argument("--out", default=None, help="also write the figures (and the whole profile report) to this JSON file")
    args = ap.parse_args(argv)
    from smalltts_amd.api import SmallTTS
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0, args.precision)
    eng.load_synthetic(7, parts=("dit", "decoder", "encoder"))
    eng.finalize()
    tts = SmallTTS(engine=eng, seed=1)
    g = np.random.default_rng(0)
    voice = tts.encode_voice(g.standard_normal((15, 64)).astype(np.float32))
    toks = [[int(t) for t in g.integers(1, 198, size=30)] for _ in range(8)]
    durs, ns = [10.0] * 8, [75] * 8
    out = {"shape": "8 pieces x 75 frames x 30 tokens, R 15", "precision": args.precision}

    if args.only == "profile":
        profile_run(args, eng, tts, toks, ns, voice, out)
    else:
        wall_run(args, tts, toks, durs, voice, out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


def profile_run(args, eng, tts, toks, ns, voice, out):
    kw = dict(frames=ns, voices=[voice] * 8, seeds=list(range(100, 108)), repair=1, return_repair=True)
    for _ in range(args.warmup):
        mended = tts.synthesize_batch(None, toks, None, **kw)[1]
    torch.cuda.synchronize()
    eng.profile(True)
    for _ in range(args.profile_reps):
        tts.synthesize_batch(None, toks, None, **kw)
    torch.cuda.synchronize()
    report = eng.profile_report()
    eng.profile(False)
    out["profile_reps"] = args.profile_reps
    out["plan"] = [[int(v) for v in m[1][0]] for m in mended]       # what the rounds had to do: (bad tokens, freed frames) per row
    out["kept"] = [int(m[0][0]) for m in mended]
    out["kernels"] = kernel_lines(report)
    out["report"] = report
    print(f"[plan at the defaults] (bad, free) per row {out['plan']}, kept {out['kept']}")
    for name, e in out["kernels"].items():
        print(f"[profile, {args.profile_reps} calls of synthesize_batch(8 rows, repair=1)] {name}: {e['launches']} launches, "
              f"{e['us_per_launch']:.2f} us each")


def wall_run(args, tts, toks, durs, voice, out):
    variants = {"no repair": {}}
    if not args.plain_only:
        variants.update({"repair=1": {"repair": 1}, "takes=2": {"takes": 2}, "takes=2, repair=1": {"takes": 2, "repair": 1}})
    call = lambda v: tts.synthesize_long(voice, token_lists=toks, durations=durs, seed=3, **variants[v])
    for v in variants:
        for _ in range(args.warmup):
            call(v)
    times = {v: [] for v in variants}
    for _ in range(args.reps):
        for v in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(v)
            times[v].append((time.perf_counter() - t0) * 1e3)
    out["synthesize_long_ms"] = {}
    for v, t in times.items():
        out["synthesize_long_ms"][v] = {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
        print(f"[synthesize_long, {args.reps} calls] {v}: median {statistics.median(t):.2f} ms ({min(t):.2f} - {max(t):.2f})")


if __name__ == "__main__":
    main()
