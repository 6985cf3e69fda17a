"""Shared argument handling for the CLI surface (tryme / clone / batch)."""
import argparse
import json

import numpy as np

from ..audio import DELIVER_RATES, read_wav, resample_hq, write_wav, write_wav_pcm16
from ..phonemes import get_token_ids, parse_tokens_arg


def add_engine_args(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("--weights", default=None, help="weight file | checkpoint .pt | synthetic:<seed>")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--precision", default="f16", help="f16 (mixed, default) | bf16x3 (fp32-class) | bf16, optionally with site overrides")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--tokens", default=None, help="pre-tokenised phoneme ids (comma/space separated or JSON)")
    ap.add_argument("--tokenizer", default="espeak", choices=["espeak", "chars"])


def add_delivery_args(ap: argparse.ArgumentParser) -> None:
    """--rate / --encoding: the output leaves the engine resampled and encoded on the device (api.Delivery)."""
    ap.add_argument("--rate", type=int, default=None, choices=DELIVER_RATES, help="output sample rate (default 24000)")
    ap.add_argument("--encoding", default=None, choices=["pcm16", "mulaw", "alaw"],
                    help="output WAV encoding: pcm16 (default), or G.711 mu-law / A-law (8 bits)")


def delivery_for(args):
    """-> None (neither flag: the output is written as it always was) or the api.Delivery the flags ask for."""
    from ..api import Delivery
    if args.rate is None and args.encoding is None:
        return None
    return Delivery(args.rate or 24_000, args.encoding or "pcm16")


def key_arg(text: str) -> int:
    """A watermark key on the command line: decimal, or 0x... hexadecimal."""
    return int(text, 0)


def add_watermark_args(ap: argparse.ArgumentParser) -> None:
    """--watermark KEY [--watermark-strength S]: the output is marked on the device (api.Watermark)."""
    ap.add_argument("--watermark", type=key_arg, default=None, metavar="KEY",
                    help="mark the output with this integer key (24000 Hz PCM16 only); scripts.detect finds it again")
    ap.add_argument("--watermark-strength", type=float, default=None, metavar="S", help="mark amplitude relative to the signal (default 0.02)")


def watermark_for(ap: argparse.ArgumentParser, args, dv):
    """-> (None or the api.Watermark the flags ask for, the Delivery to use: Delivery(24000, "pcm16") where a mark has none)."""
    from ..api import Delivery, Watermark
    if args.watermark is None:
        if args.watermark_strength is not None:
            ap.error("--watermark-strength belongs to --watermark")
        return None, dv
    if dv is None:
        dv = Delivery(24_000, "pcm16")
    if dv.rate != 24_000 or dv.encoding != "pcm16":
        ap.error("--watermark needs 24000 Hz PCM16 output: the mark would not survive resampling or G.711")
    try:
        return Watermark(args.watermark, 0.02 if args.watermark_strength is None else args.watermark_strength), dv
    except ValueError as e:
        ap.error(str(e))


def pcm16_host(audio) -> np.ndarray:
    """float [-1, 1] -> int16 by write_wav_pcm16's arithmetic (clamp, x 32767, round to nearest even)."""
    a = np.asarray(audio, dtype=np.float32).reshape(-1)
    return np.round(np.clip(a, -1.0, 1.0) * 32767.0).astype(np.int16)


def write_output(path: str, audio, delivery=None) -> None:
    """A synthesis result to a WAV: float samples at 24 kHz as PCM_16 (the host writer), or what a Delivery returned, as it is."""
    a = np.asarray(audio).reshape(-1)
    if delivery is None:
        write_wav_pcm16(path, a, 24_000)
    else:
        write_wav(path, a, delivery.rate, delivery.encoding)


def tokens_for(args, text: str):
    if args.tokens:
        if args.tokens.strip().startswith("["):
            return [int(t) for t in json.loads(args.tokens)]
        return parse_tokens_arg(args.tokens)
    return get_token_ids(text, backend=args.tokenizer)


def load_reference_wav(path: str, engine=None) -> np.ndarray:
    """-> mono float32 @ 24 kHz, shape (1, 1, S) (clone.py:29-33).  With an engine the resampling runs on the
    device (smtts_resample_poly); the host numpy restatement is the fallback-free CPU path of the same filter."""
    y, sr = read_wav(path)
    if y.ndim == 2:
        y = y.mean(axis=1)
    if engine is not None:
        y = engine.resample(y.astype(np.float32), sr, 24_000).cpu().numpy()
    else:
        y = resample_hq(y.astype(np.float32), sr, 24_000)
    return y[None, None, :]
