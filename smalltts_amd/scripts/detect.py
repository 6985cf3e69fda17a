"""python -m smalltts_amd.scripts.detect --wav f.wav --key K [--max-offset N] [--threshold T] [--device D]
Looks for the watermark of key K (api.Watermark) in a 24 kHz WAV: prints z, the offset and the verdict; exit status 0 if
the mark is present, 1 if not.  --max-offset N: the file may have lost up to N samples at its front (every offset is tried on the
device).  Needs the GPU and no weights.  A file at another rate is refused: the detector is specified for 24 kHz f32 / PCM16 only."""
import argparse
import sys
import wave

import numpy as np

from ..audio import read_wav
from ._common import key_arg


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="detect a smalltts_amd watermark in a 24 kHz WAV")
    ap.add_argument("--wav", required=True, help="the file to examine (24000 Hz; PCM16 or float)")
    ap.add_argument("--key", required=True, type=key_arg, help="the integer key the audio was marked with (decimal or 0x...)")
    ap.add_argument("--max-offset", type=int, default=0, metavar="N", help="samples the file may have lost at its front (default 0)")
    ap.add_argument("--threshold", type=float, default=6.0, metavar="T", help="z at or above which the mark counts as present (default 6.0)")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if not 0 <= args.key < 2 ** 64:
        ap.error("--key must be in [0, 2^64)")
    if not 0 <= args.max_offset <= 2 ** 40:
        ap.error("--max-offset must be in [0, 2^40]")
    if not args.threshold == args.threshold:
        ap.error("--threshold must be a number")
    return args


def load(path: str):
    """-> (mono samples, rate): int16 as stored for a PCM16 file (the detector divides by 32767), float32 otherwise."""
    try:
        with wave.open(path, "rb") as w:
            if w.getsampwidth() == 2 and w.getcomptype() == "NONE":
                x = np.frombuffer(w.readframes(w.getnframes()), "<i2").reshape(-1, w.getnchannels())
                if x.shape[1] == 1:
                    return x[:, 0].astype(np.int16), w.getframerate()
    except (wave.Error, EOFError):
        pass
    y, sr = read_wav(path)
    return (y.mean(axis=1) if y.ndim == 2 else y).astype(np.float32), sr


def main(argv=None) -> int:
    args = parse_args(argv)
    x, sr = load(args.wav)
    if sr != 24_000:
        raise SystemExit(f"{args.wav}: {sr} Hz; the detector is specified for 24000 Hz only")
    from ..api import detect_watermark
    from ..engine import HipEngine
    z, off, present = detect_watermark(HipEngine(args.device), x, args.key, max_offset=args.max_offset, threshold=args.threshold)[0]
    print(f"z = {z:.2f} at offset {off}: {'present' if present else 'absent'} (threshold {args.threshold:g})")
    return 0 if present else 1


if __name__ == "__main__":
    sys.exit(main())
