"""python -m smalltts_amd.scripts.pitch --wav rec.wav [--words in.json] --out f0.json [--csv f0.csv] [--fmin 60] [--fmax 400]
The F0 track of a recording, on the device (api.pitch_track_wav): a normalised cross-correlation score per frame and
candidate lag, and the best path through them (Viterbi); one value per 10 ms.  Needs no weights and no text.
--out: {"hop", "sr", "f0": [Hz, 0 where unvoiced], "strength": [the score at the chosen lag]} and, with --words, "words": the word
rows of scripts/align.py's --words file (either of its two shapes), each with f0_median, f0_min, f0_max (Hz over the word's voiced
frames, null where it has none) and voiced (the share of its frames that is voiced).
--csv: one line per frame: time in seconds, f0, strength.
The tracker's constants are design choices checked on synthetic signals only (tones, noise, silence); they were not tuned on speech,
and nothing is claimed about its accuracy on speech."""
import argparse
import json
from pathlib import Path

from ..api import pitch_track_wav
from ..audio import read_wav
from ..engine import HipEngine
from ..options import Pitch
from .align import words_json
from .retime import target_words


def pitch_json(track, stats=None) -> str:
    """A PitchTrack and pitch_track's word list -> the --out file."""
    doc = {"hop": int(track.hop), "sr": int(track.sr), "f0": [round(float(v), 3) for v in track.f0],
           "strength": [round(float(v), 4) for v in track.strength]}
    if stats is not None:
        doc["words"] = json.loads(words_json([w for w, _s in stats], [s for _w, s in stats]))
    return json.dumps(doc, ensure_ascii=False, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--wav", required=True, help="a mono recording of any length")
    ap.add_argument("--words", default=None, metavar="IN.json", help="a --words file of scripts/align.py: f0 statistics per word")
    ap.add_argument("--out", required=True, metavar="F0.json")
    ap.add_argument("--csv", default=None, metavar="F0.csv", help="also one line per frame: seconds, f0, strength")
    ap.add_argument("--fmin", type=float, default=60.0, help="the lowest f0 searched, Hz")
    ap.add_argument("--fmax", type=float, default=400.0, help="the highest f0 searched, Hz")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    try:
        pt = Pitch(fmin=args.fmin, fmax=args.fmax)
        words = target_words(args.words) if args.words else None
    except (ValueError, TypeError, KeyError) as e:
        ap.error(str(e))
    y, sr = read_wav(args.wav)
    if y.ndim == 2:
        y = y.mean(axis=1)
    res = pitch_track_wav(HipEngine(args.device), y, sr, pt, words)
    track, stats = res if words is not None else (res, None)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(pitch_json(track, stats), encoding="utf-8")
    voiced = int((track.f0 > 0).sum())
    print(f"{args.out} ({track.f0.size} frames, {voiced} voiced)")
    if args.csv:
        Path(args.csv).parent.mkdir(parents=True, exist_ok=True)
        Path(args.csv).write_text("".join(f"{f * track.hop / track.sr:.4f},{v:.3f},{s:.4f}\n"
                                          for f, (v, s) in enumerate(zip(track.f0, track.strength))), encoding="utf-8")
        print(args.csv)


if __name__ == "__main__":
    main()
