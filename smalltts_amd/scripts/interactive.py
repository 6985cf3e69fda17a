"""python -m smalltts_amd.scripts.interactive [--wav ref.wav]   (reference src/scripts/infer/interactive.py:17-60)

Type a line, get speech: every line is tokenised, given estimate_duration(line) seconds and synthesised with the loaded
reference voice; prints generation time and the real-time factor like the reference (`gen 0.02s, 480.0x rt`).  The reference
plays through `sounddevice` and draws with `rich`; both are optional here — without sounddevice every utterance is written to
out/interactive_NNN.wav instead.  --stream decodes in chunks (SmallTTS.synthesize_stream) and prints the time to the first chunk next
to the total (`gen 0.02s, first chunk 0.01s, 480.0x rt`); with it --rate / --encoding make the chunks leave the device at that rate
and encoding (api.Delivery), and the file written is a WAV of that format; --watermark KEY [--watermark-strength S] marks the chunks
on the device (api.Watermark; 24000 Hz PCM16 only)."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

from ..api import Encoder, SmallTTS, estimate_duration
from ._common import (add_delivery_args, add_engine_args, add_watermark_args, delivery_for, load_reference_wav, tokens_for, watermark_for,
                      write_output)


def main(argv=None, lines=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--wav", type=str, help="reference audio file")
    ap.add_argument("--ref-latents", default="assets/tryme/latents.npy", help="(R,64) float32 .npy reference voice (no --wav)")
    ap.add_argument("--outdir", default="out")
    ap.add_argument("--stream", action="store_true", help="decode in chunks; also print the time to the first chunk")
    add_engine_args(ap)
    add_delivery_args(ap)
    add_watermark_args(ap)
    args = ap.parse_args(argv)
    wm, dv = watermark_for(ap, args, delivery_for(args))
    if dv is not None and not args.stream:
        ap.error("--rate / --encoding / --watermark belong to --stream")
    try:
        import sounddevice as sd
    except Exception:
        sd = None
    print("smalltts interactive\ntype and press enter. ctrl-c to exit.\nloading model")
    t0 = time.perf_counter()
    kw = dict(weights=args.weights, device=args.device, precision=args.precision)
    model = SmallTTS(num_steps=args.steps, seed=args.seed, **kw)
    if args.wav:
        enc = Encoder(**kw)
        x = torch.from_numpy(load_reference_wav(args.wav, enc.engine))
        ref_latents = enc.encode_reference(x)[0].cpu().numpy()        # cached per voice (interactive.py:34)
    elif Path(args.ref_latents).exists():
        ref_latents = np.load(args.ref_latents).astype(np.float32)
    else:
        print(f"{args.ref_latents} not found: using a seeded random reference voice")
        ref_latents = np.random.default_rng(0).standard_normal((15, 64)).astype(np.float32)
    Path(args.outdir).mkdir(parents=True, exist_ok=True)
    first, n = True, 0
    src = iter(lines) if lines is not None else None
    while True:
        try:
            s = (next(src) if src is not None else input(">> ")).strip()
        except (EOFError, KeyboardInterrupt, StopIteration):
            break
        if not s:
            continue
        st = time.perf_counter()
        tokens = tokens_for(args, s)
        t_first = None
        if args.stream:
            chunks = []
            for c in model.synthesize_stream(ref_latents, tokens, estimate_duration(s), **({} if dv is None else {"deliver": dv, "watermark": wm})):
                t_first = time.perf_counter() - st if t_first is None else t_first
                chunks.append(c)
            audio = np.concatenate(chunks, axis=1)
        else:
            audio = model.synthesize(ref_latents, tokens, estimate_duration(s))
        dt = time.perf_counter() - st
        dur = audio.shape[-1] / float(24_000 if dv is None else dv.rate)
        rtf = dur / dt if dt > 0 else 0.0
        if first:
            print(f"gen {dt:.2f}s (+{time.perf_counter() - t0 - dt:.2f}s warmup), " + (f"first chunk {t_first:.2f}s, " if t_first is not None else "")
                  + f"{rtf:.1f}x rt")
            first = False
        else:
            print(f"gen {dt:.2f}s, " + (f"first chunk {t_first:.2f}s, " if t_first is not None else "") + f"{rtf:.1f}x rt")
        a = audio.squeeze()
        if sd is not None and dv is None:
            sd.play(a, 24_000)
            sd.wait()
        else:
            path = str(Path(args.outdir) / f"interactive_{n:03d}.wav")
            write_output(path, a, dv)
            print(path)
        n += 1
    return n


if __name__ == "__main__":
    sys.exit(0 if main() >= 0 else 1)
