"""python tools/ctc_align_long_bench.py [--reps 10] [--out FILE.json]
The time per launch of smtts_ctc_align_long at (T, P) = (900, 198), (8192, 2000) and (65536, 16383), one row each, next to
smtts_ctc_align at (900, 198) in the same process (NOTEBOOK "Long alignment"), by the library's own per-kernel profiler (HIP
events around every launch).  log-softmax of seeded noise over 64 classes, tokens without equal neighbours, the row full length, so
every shape is feasible and is traced back; 5 x --reps launches at the small shape, --reps at the middle one, --reps / 3 at the limit."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = ((900, 198), (8192, 2000), (65536, 16383))
NC = 64


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0)                                          # the CTC entries need no weights
    g = torch.Generator().manual_seed(0)
    out = {"classes": NC, "rows": 1, "reps": args.reps, "us_per_launch": {}, "launches": {}}
    for T, P in SHAPES:
        logp = torch.randn(1, T, NC, generator=g).log_softmax(-1).to(eng.device)
        tok = (1 + torch.arange(P) % (NC - 1)).to(torch.int32)[None].contiguous().to(eng.device)
        entries = [("ctc_align_long", eng.ctc_align_long)] + ([("ctc_align", eng.ctc_align)] if T <= 1024 and P <= 198 else [])
        reps = 5 * args.reps if T <= 1024 else args.reps if T < 65536 else max(3, args.reps // 3)
        for _name, fn in entries:
            for _ in range(2):
                fn(logp, [T], tok, [0], [P], frames=True)
        torch.cuda.synchronize()
        eng.profile(True)
        for _ in range(reps):                                   # alternating, so that drift hits both alike
            for _name, fn in entries:
                score = fn(logp, [T], tok, [0], [P], frames=True)[2]
        torch.cuda.synchronize()
        report = eng.profile_report()
        eng.profile(False)
        assert bool(torch.isfinite(score).all()), (T, P)
        for e in report:
            if e["name"] in dict(entries):
                us = round(1e3 * e["ms"] / max(e["launches"], 1), 1)
                out["us_per_launch"][f"{e['name']} T{T} P{P}"] = us
                out["launches"][f"{e['name']} T{T} P{P}"] = e["launches"]
                print(f"[profile, 1 row x {T} frames x {P} tokens, C {NC}] {e['name']}: {e['launches']} launches, {us:.1f} us each")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
