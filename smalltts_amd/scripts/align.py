"""python -m smalltts_amd.scripts.align --wav rec.wav --text "..." --words out.json [--srt out.srt]
python -m smalltts_amd.scripts.align --take in.npz --out-take out.npz
Forced alignment by the latent phoneme recogniser (api.SmallTTS.align_wav / realign): the best CTC path of the phonemes
through the recogniser's reading of the audio's latents, 33.3 ms resolution (800 samples at 24 kHz).
--wav: a mono recording of at most 30 s and what it says (--text through the tokeniser, or --tokens) -> --words, a JSON list of
{index, kind, phonemes, start, end (samples at 24 kHz), start_s, end_s, confidence}; confidence is the path's mean log-probability per
frame over the group's tokens, null where the recording could not be aligned.  --srt: one subtitle cue per word group.
--long: --wav of any length up to 36 min goes through api.SmallTTS.align_wav_long (the recogniser in 30 s windows, the path by
smtts_ctc_align_long); --words then holds {"words": that list, "speaking_rate": {"tokens_per_second", "speech_seconds"}}
(plans.speaking_rate over the aligned phonemes, pauses over 200 ms counted as 200 ms; null where fewer than two phonemes were aligned).
--take: the pieces of a long take (scripts/longform.py --take) get the recogniser's token spans in place of the text-attention tap's,
in codec frames, and are written to --out-take with the take's join parameters unchanged: scripts/respeak.py --groups then cuts
where the recogniser heard the words.  A piece that could not be aligned keeps its spans.
--pitch: every word of --words also gets f0_median, f0_min, f0_max (Hz over its voiced frames, null where it has none) and voiced (the
share of its frames that is voiced), from the device's F0 track of the recording (api.SmallTTS.pitch_wav; its constants
were checked on synthetic signals only, not on speech).  Without the flag the file is what it always was, byte for byte.
Only the mechanism is verified: no trained recogniser checkpoint has ever been loaded, so what these times are worth is unvalidated."""
import argparse
import json
from pathlib import Path

from ..api import SAMPLE_RATE, SmallTTS, format_srt, load_take, save_take, speaking_rate
from ..audio import read_wav
from ._common import add_engine_args, tokens_for


def _words_json(words) -> str:
    fin = lambda v: float(v) if float("-inf") < float(v) < float("inf") else None
    return json.dumps([{"index": int(i), "kind": kind, "phonemes": ph, "start": int(s), "end": int(e),
                        "start_s": round(int(s) / SAMPLE_RATE, 4), "end_s": round(int(e) / SAMPLE_RATE, 4), "confidence": fin(c)}
                       for i, kind, ph, s, e, c in words], ensure_ascii=False, indent=1)


def with_stats(rows: list, stats: list) -> list:
    """The rows of a --words file, each with the four pitch statistics of its word (plans.pitch_word_stats; f0 rounded to 0.01 Hz)."""
    r2 = lambda v: None if v is None else round(float(v), 2)
    return [dict(r, f0_median=r2(s["f0_median"]), f0_min=r2(s["f0_min"]), f0_max=r2(s["f0_max"]), voiced=round(float(s["voiced"]), 4))
            for r, s in zip(rows, stats)]


def words_json(words, stats=None) -> str:
    """align_words' row -> the --words file; with `stats` (one dict per row) every word carries its pitch statistics too."""
    if stats is None:
        return _words_json(words)
    return json.dumps(with_stats(json.loads(_words_json(words)), stats), ensure_ascii=False, indent=1)


def long_json(words, spans, stats=None) -> str:
    """align_wav_long's words and spans -> the --words file of --long."""
    rate, seconds = speaking_rate(spans)
    return json.dumps({"words": json.loads(words_json(words, stats)),
                       "speaking_rate": {"tokens_per_second": round(rate, 4) if rate == rate else None, "speech_seconds": round(seconds, 4)}},
                      ensure_ascii=False, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--wav", default=None, help="a mono recording of at most 30 s")
    ap.add_argument("--text", default=None, help="what the recording says (or --tokens)")
    ap.add_argument("--words", default=None, metavar="OUT.json", help="write the time of every word / punctuation mark / [event] (33 ms resolution)")
    ap.add_argument("--srt", default=None, metavar="OUT.srt", help="write one subtitle cue per word group")
    ap.add_argument("--long", action="store_true", help="--wav of up to 36 min (align_wav_long); --words gains the speaking rate")
    ap.add_argument("--pitch", action="store_true", help="with --wav and --words: add f0_median / f0_min / f0_max / voiced to every word")
    ap.add_argument("--take", default=None, metavar="IN.npz", help="a long take (longform --take) to align again")
    ap.add_argument("--out-take", default=None, metavar="OUT.npz", help="where the take with the recogniser's spans goes")
    add_engine_args(ap)
    args = ap.parse_args(argv)
    if (args.wav is None) == (args.take is None):
        ap.error("pass either --wav or --take")
    if args.wav is not None and (not (args.text or args.tokens) or not (args.words or args.srt) or args.out_take):
        ap.error("--wav needs --text or --tokens, and --words or --srt; --out-take belongs to --take")
    if args.take is not None and (not args.out_take or args.text or args.words or args.srt):
        ap.error("--take needs --out-take; --text, --words and --srt belong to --wav")
    if args.long and args.wav is None:
        ap.error("--long belongs to --wav")
    if args.pitch and (args.wav is None or not args.words):
        ap.error("--pitch belongs to --wav and --words")
    print("loading")
    tts = SmallTTS(weights=args.weights, device=args.device, precision=args.precision, num_steps=args.steps, seed=args.seed,
                   recogniser=True)
    if args.wav is not None:
        y, sr = read_wav(args.wav)
        if y.ndim == 2:
            y = y.mean(axis=1)
        try:
            if args.long:
                words, spans = tts.align_wav_long(y, sr, tokens_for(args, args.text or ""), return_spans=True)
            else:
                words = tts.align_wav(y, sr, tokens_for(args, args.text or ""))
        except ValueError as e:
            ap.error(str(e))
        if args.words:
            stats = [s for _w, s in tts.pitch_wav(y, sr, words=words)[1]] if args.pitch else None
            Path(args.words).parent.mkdir(parents=True, exist_ok=True)
            Path(args.words).write_text(long_json(words, spans, stats) if args.long else words_json(words, stats), encoding="utf-8")
            print(f"{args.words} ({len(words)} word groups)")
        if args.srt:
            Path(args.srt).parent.mkdir(parents=True, exist_ok=True)
            Path(args.srt).write_text(format_srt([(s, e, ph) for _i, _kind, ph, s, e, _c in words]), encoding="utf-8")
            print(args.srt)
        return
    pieces, join = load_take(args.take)
    out = tts.realign(pieces)
    Path(args.out_take).parent.mkdir(parents=True, exist_ok=True)
    save_take(args.out_take, out, **join)
    print(f"{args.out_take} ({len(out)} pieces)")


if __name__ == "__main__":
    main()
