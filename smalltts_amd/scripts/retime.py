"""python -m smalltts_amd.scripts.retime --wav in.wav (--text "..." | --tokens ...) (--speed X | --duration S | --to-words target.json)
                                       [--long] --out out.wav [--words out.json] [--srt out.srt]
Retimes a recording on the device (api.SmallTTS.retime_wav): WSOLA, the pitch is kept.  The recording is aligned first
(scripts/align.py's aligner; --long for more than 30 s, up to 36 min), so the text is needed for every target.
--speed X: X times as fast.  --duration S: exactly round(S * 24000) samples.  --to-words target.json: every word is laid where the
target's word of the same index lies; target.json is a --words file of scripts/align.py, in either of its two shapes (the list, or
--long's {"words": [...]}), e.g. the alignment of another reading of the same text.  A word whose rate would leave [--min-rate,
--max-rate] keeps its start and has its length clamped; the indices of such words are printed.
--out: PCM16 at 24 kHz.  --words: where every word lies in the result, in scripts/align.py's format; --srt: one cue per word group.
How retimed speech sounds is untested: only signal properties are (a unit map returns the input, a tone keeps its pitch)."""
import argparse
import json
from pathlib import Path

from ..api import Retime, SmallTTS, format_srt
from ..audio import read_wav
from ._common import add_engine_args, tokens_for, write_output
from .align import words_json


def target_words(path: str) -> list:
    """A --words file of scripts/align.py (the list, or --long's object) -> rows as align_words returns them."""
    doc = json.loads(Path(path).read_text(encoding="utf-8"))
    rows = doc["words"] if isinstance(doc, dict) else doc
    conf = lambda v: float("-inf") if v is None else float(v)
    return [(int(r["index"]), r["kind"], r.get("phonemes", ""), int(r["start"]), int(r["end"]), conf(r.get("confidence"))) for r in rows]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--wav", required=True, help="a mono recording")
    ap.add_argument("--text", default=None, help="what the recording says (or --tokens)")
    ap.add_argument("--speed", type=float, default=None, metavar="X", help="X times as fast")
    ap.add_argument("--duration", type=float, default=None, metavar="S", help="exactly S seconds")
    ap.add_argument("--to-words", default=None, metavar="TARGET.json", help="a --words file of scripts/align.py: where the words shall lie")
    ap.add_argument("--min-rate", type=float, default=0.5, help="with --to-words: the slowest a word may run (source per output sample)")
    ap.add_argument("--max-rate", type=float, default=2.0, help="with --to-words: the fastest a word may run")
    ap.add_argument("--long", action="store_true", help="a recording of more than 30 s, up to 36 min (align_wav_long)")
    ap.add_argument("--out", required=True, metavar="OUT.wav")
    ap.add_argument("--words", default=None, metavar="OUT.json", help="write where every word lies in the result")
    ap.add_argument("--srt", default=None, metavar="OUT.srt", help="write one subtitle cue per word group of the result")
    add_engine_args(ap)
    args = ap.parse_args(argv)
    if (args.speed is not None) + (args.duration is not None) + (args.to_words is not None) != 1:
        ap.error("pass exactly one of --speed, --duration and --to-words")
    if not (args.text or args.tokens):
        ap.error("--wav needs --text or --tokens: the recording is aligned before it is retimed")
    try:
        rt = Retime(speed=args.speed, duration=args.duration, to_words=target_words(args.to_words) if args.to_words else None,
                    min_rate=args.min_rate, max_rate=args.max_rate)
    except (ValueError, TypeError, KeyError) as e:
        ap.error(str(e))
    print("loading")
    tts = SmallTTS(weights=args.weights, device=args.device, precision=args.precision, num_steps=args.steps, seed=args.seed,
                   recogniser=True)
    y, sr = read_wav(args.wav)
    if y.ndim == 2:
        y = y.mean(axis=1)
    try:
        audio, words, clamped = tts.retime_wav(y, sr, tokens_for(args, args.text or ""), rt, long=args.long)
    except ValueError as e:
        ap.error(str(e))
    if clamped:
        print("clamped words: " + " ".join(str(i) for i in clamped))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    write_output(args.out, audio.squeeze(0))
    print(f"{args.out} ({audio.shape[1] / 24_000:.3f}s)")
    if args.words:
        Path(args.words).parent.mkdir(parents=True, exist_ok=True)
        Path(args.words).write_text(words_json(words), encoding="utf-8")
        print(f"{args.words} ({len(words)} word groups)")
    if args.srt:
        Path(args.srt).parent.mkdir(parents=True, exist_ok=True)
        Path(args.srt).write_text(format_srt([(s, e, ph) for _i, _kind, ph, s, e, _c in words]), encoding="utf-8")
        print(args.srt)


if __name__ == "__main__":
    main()
