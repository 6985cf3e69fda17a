"""python -m smalltts_amd.scripts.clone --wav ref.wav --text "..." [--duration S] [--out out/clone.wav] [--trim] [--trim-ref]
[--rate 8000 --encoding mulaw] [--watermark KEY [--watermark-strength S]]
(reference src/scripts/infer/clone.py: read wav -> mono -> 24 kHz -> codec encode -> synthesize)"""
import argparse
from pathlib import Path

import torch

from ..api import HOP_SIZE, Encoder, Endpointing, SmallTTS, estimate_duration
from ._common import (add_delivery_args, add_engine_args, add_watermark_args, delivery_for, load_reference_wav, tokens_for, watermark_for,
                      write_output)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--wav", required=True, help="reference audio file")
    ap.add_argument("--text", required=True, help="text to speak")
    ap.add_argument("--duration", type=float, default=None, help="duration in seconds (auto if omitted)")
    ap.add_argument("--out", default="out/clone.wav")
    ap.add_argument("--trim", action="store_true", help="write only the speech: the ends the endpoint kernels find, not the whole duration")
    ap.add_argument("--trim-ref", action="store_true", help="cut the reference clip to its speech (whole codec hops) before encoding it")
    add_engine_args(ap)
    add_delivery_args(ap)
    add_watermark_args(ap)
    args = ap.parse_args(argv)
    wm, dv = watermark_for(ap, args, delivery_for(args))
    if dv is not None and args.trim:
        ap.error("--rate / --encoding / --watermark do not go with --trim")
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    print("loading")
    kw = dict(weights=args.weights, device=args.device, precision=args.precision)
    enc = Encoder(**kw)
    x = load_reference_wav(args.wav, enc.engine)
    print("encoding reference audio")
    tts = SmallTTS(num_steps=args.steps, seed=args.seed, **kw)
    if args.trim_ref:
        seg = enc.engine.endpoints(torch.from_numpy(x).to(enc.engine.device).contiguous(), None, Endpointing(), lens=[x.shape[-1]])[0].cpu()
        start, n = int(seg[0, 0]), int(seg[0, 1])
        if n == 0:
            raise SystemExit("--trim-ref: no speech found in the reference clip")
        n = max(HOP_SIZE, n // HOP_SIZE * HOP_SIZE)      # as SmallTTS.encode_voice_wav(trim=True) cuts it
        start = max(0, min(start, x.shape[-1] - n))
        x = x[..., start:start + n]
    ref_latents = enc.encode_reference(torch.from_numpy(x))[0].numpy()
    tokens = tokens_for(args, args.text)
    duration = args.duration or estimate_duration(args.text)
    print(f"generating ({duration:.1f}s)")
    audio = (tts.synthesize_batch([ref_latents], [tokens], [duration], trim=True)[0] if args.trim
             else tts.synthesize(ref_latents, tokens, duration) if dv is None
             else tts.synthesize_batch([ref_latents], [tokens], [duration], deliver=dv, watermark=wm)[0])
    write_output(args.out, audio, dv)
    print(args.out)


if __name__ == "__main__":
    main()
