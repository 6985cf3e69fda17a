"""python tools/sv_bench.py --only profile|wall [--reps 15] [--warmup 3] [--profile-reps 20] [--precision f16] [--out FILE.json]
What the speaker term of the takes costs at the benchmark shape (8 pieces x 75 frames, reference 15 frames, 30 tokens, 4 DMD steps, the
full-size codec, seeded synthetic weights), two measurements, each in a run of its own (the profiler's events slow the
host, so the wall times are taken in a process that never switched it on):
* the library's own per-kernel profiler (HIP events around every launch) over `--profile-reps` calls of
  synthesize_batch(takes=Takes(4, sv=1.0)): 8 rows x 4 takes = 32 sampler rows of 75 frames, one call at a time; the lines of the
  verifier's kernels and the takes' own kernels are printed, and the fraction of the f32-input MFMA roof (157 TFLOP/s) sv_tdnn reaches;
* the wall time of synthesize_long on the same eight pieces with takes = 4, without and with the speaker term: a host clock around the
  call, which ends in the copy of the waveform to the host (a synchronise); `--warmup` calls of every variant first, then the variants
  alternate call by call so that drift hits them alike; median (min - max) of `--reps` calls.
python tools/sv_bench.py --find-seed: the first (weight w, base seed s), w in 4, 16, 64 and s in 0 .. 31, at which synthesize_batch(3
rows seeded s, s + 1, s + 2, takes=3) keeps another take with sv = w than without, at the shapes of tests/test_takes_sv_gpu.py (which
names that pair)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KERNELS = ("sv_", "take_scores", "take_select", "align_path", "attn_text_mass")
MFMA_F32_ROOF = 157e12   # flop/s of the f32-input MFMA on an MI355X


def kernel_lines(report):
    """The entries of a profile report (a list of {name, launches, ms, ...}) that name one of KERNELS, with the time per launch."""
    return {e["name"]: dict(e, us_per_launch=round(1e3 * e["ms"] / max(e["launches"], 1), 3)) for e in report
            if any(k in e["name"] for k in KERNELS)}


def find_seed():
    from smalltts_amd.api import SmallTTS, Takes
    from smalltts_amd.engine import HipEngine
    from smalltts_amd.weights import CodecSpec
    spec = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))
    eng = HipEngine(0, "bf16x3")
    eng.load_synthetic(11, parts=("dit", "decoder", "encoder", "sv"), codec_spec=spec)
    eng.finalize()
    tts = SmallTTS(engine=eng, seed=1, verifier=True)
    g = np.random.default_rng(0)
    voices = [tts.encode_voice(g.standard_normal((r, 64)).astype(np.float32)) for r in (6, 9, 7)]
    toks = [[1, 2, 3, 4, 5, 6], [10, 20, 30, 40, 50, 60, 70, 80, 90, 100, 110, 120], [7, 8, 9, 17, 18, 19, 27, 28, 29]]
    for w in (4.0, 16.0, 64.0):
        for s in range(32):
            kw = dict(frames=[9, 20, 14], voices=voices, seeds=[s, s + 1, s + 2], return_takes=True)
            a = tts.synthesize_batch(None, toks, None, takes=Takes(3), **kw)[-1]
            b = tts.synthesize_batch(None, toks, None, takes=Takes(3, sv=w), **kw)[-1]
            wa, wb = [t[0] for t in a], [t[0] for t in b]
            print(f"sv {w} seed {s}: winners without the term {wa}, with it {wb}; cosines {[np.round(t[-1], 4).tolist() for t in b]}")
            if wa != wb:
                return w, s
    print("no weight among 4, 16, 64 and seed among 0 .. 31 changes a winner")
    return None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["profile", "wall"], help="which of the two measurements this run takes")
    ap.add_argument("--find-seed", action="store_true")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-reps", type=int, default=20)
    ap.add_argument("--precision", default="f16")
    ap.add_argument("--out", default=None, help="also write the figures (and the whole profile report) to this JSON file")
    args = ap.parse_args(argv)
    if args.find_seed:
        return find_seed()
    if args.only is None:
        ap.error("--only profile | wall, or --find-seed")
    from smalltts_amd.api import SmallTTS
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0, args.precision)
    eng.load_synthetic(7, parts=("dit", "decoder", "encoder", "sv"))
    eng.finalize()
    tts = SmallTTS(engine=eng, seed=1, verifier=True)
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
    from smalltts_amd.api import Takes
    kw = dict(frames=ns, voices=[voice] * 8, seeds=list(range(100, 108)), takes=Takes(4, sv=1.0))
    for _ in range(args.warmup):
        tts.synthesize_batch(None, toks, None, **kw)
    torch.cuda.synchronize()
    eng.profile(True)
    for _ in range(args.profile_reps):
        tts.synthesize_batch(None, toks, None, **kw)
    torch.cuda.synchronize()
    report = eng.profile_report()
    eng.profile(False)
    out["profile_reps"] = args.profile_reps
    out["kernels"] = kernel_lines(report)
    out["report"] = report
    sv_ms = sum(e["ms"] for n, e in out["kernels"].items() if "sv_" in n) / args.profile_reps
    out["sv_term_kernel_ms_per_call"] = round(sv_ms, 4)
    tdnn = [e for n, e in out["kernels"].items() if n.endswith("sv_tdnn")]
    if tdnn and tdnn[0]["ms"] > 0:
        out["sv_tdnn_fraction_of_f32_mfma_roof"] = round(tdnn[0]["flops"] / (tdnn[0]["ms"] * 1e-3) / MFMA_F32_ROOF, 4)
        print(f"[profile] sv_tdnn: {tdnn[0]['flops'] / (tdnn[0]['ms'] * 1e-3) / 1e12:.1f} TFLOP/s over its launches, "
              f"{100 * out['sv_tdnn_fraction_of_f32_mfma_roof']:.1f} % of the f32-input MFMA roof")
    for name, e in out["kernels"].items():
        print(f"[profile, {args.profile_reps} calls of synthesize_batch(8 rows, takes=Takes(4, sv=1.0))] {name}: {e['launches']} launches, "
              f"{e['us_per_launch']:.2f} us each")
    print(f"[profile] verifier kernels: {sv_ms:.3f} ms per call")


def wall_run(args, tts, toks, durs, voice, out):
    from smalltts_amd.api import Takes
    variants = {"takes=4": {"takes": 4}, "takes=4 sv=1": {"takes": Takes(4, sv=1.0)}}
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
