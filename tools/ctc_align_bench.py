"""python tools/ctc_align_bench.py [--rows 32] [--frames 300] [--tokens 30] [--reps 50] [--out FILE.json]
The time per launch of smtts_ctc_align next to smtts_ctc_score on the same buffers (NOTEBOOK), by the library's own
per-kernel profiler (HIP events around every launch): log-softmax of seeded noise, random tokens, every row full length.  The default
shape is what Takes(4, ctc=) gives the score at the benchmark shape: 32 rows x 300 recogniser frames x 30 tokens."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--tokens", type=int, default=30)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0)                                          # the CTC entries need no weights
    B, T, P = args.rows, args.frames, args.tokens
    g = torch.Generator().manual_seed(0)
    logp = torch.randn(B, T, 198, generator=g).log_softmax(-1).to(eng.device)
    tok = torch.randint(1, 198, (B, P), generator=g).to(torch.int32).to(eng.device)
    ts, p0, p1 = [T] * B, [0] * B, [P] * B
    for _ in range(5):
        eng.ctc_score(logp, ts, tok, p0, p1)
        eng.ctc_align(logp, ts, tok, p0, p1, frames=True)
    torch.cuda.synchronize()
    eng.profile(True)
    for _ in range(args.reps):                                  # alternating, so that drift hits both alike
        eng.ctc_score(logp, ts, tok, p0, p1)
        eng.ctc_align(logp, ts, tok, p0, p1, frames=True)
    torch.cuda.synchronize()
    report = eng.profile_report()
    eng.profile(False)
    out = {"shape": f"{B} rows x {T} frames x {P} tokens, C 198", "reps": args.reps}
    for e in report:
        if e["name"] in ("ctc_score", "ctc_align"):
            out[e["name"] + "_us_per_launch"] = round(1e3 * e["ms"] / max(e["launches"], 1), 3)
            print(f"[profile, {out['shape']}] {e['name']}: {e['launches']} launches, {out[e['name'] + '_us_per_launch']:.2f} us each")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
