"""python -m smalltts_amd.scripts.longform --wav ref.wav --text-file text.txt [--out out/longform.wav] [--trim [--level DBFS]]
A whole text in one cloned voice: the voice is encoded once, the text is cut into utterance-sized pieces (api.split_text), the
pieces run as batches in flight and are joined on the device (api.SmallTTS.synthesize_long).
Without espeak: --tokens-file (one comma-separated token list per line = one piece) with --durations (seconds, one per line).
--words out.json: when every word / punctuation mark / [event] is spoken (from the DiT's text attention: api.Alignment, default
selection unvalidated on trained weights; resolution one codec frame = 133 ms).  --srt out.srt: one subtitle cue per piece, and
next to it out.words.srt with one cue per word group.  --take OUT.npz: the pieces (tokens, latents, seeds; with --words also each
piece's token spans) and the join parameters, what scripts/respeak.py re-speaks a span of and renders again.
--takes K: every piece is sampled K times and the take whose text alignment scores best is kept (api.Takes; what the score is worth is
unvalidated on trained weights); with --words the JSON becomes {"words": [...], "takes": [{piece, winner, seed, totals}, ...]}.
--ctc W (with --takes; loads the latent phoneme recogniser, api.SmallTTS(recogniser=True)): the score gains W * CTC nll / tokens of the
recogniser's reading of every take (api.Takes(ctc=); unvalidated like the rest of the score, not with --repair), and every
entry of "takes" in the --words JSON gains "nll", the K values.
--sv W (with --takes; loads the latent speaker verifier, api.SmallTTS(verifier=True)): the score gains W * (1 - cosine) of every take's
speaker embedding with the reference voice's (api.Takes(sv=); unvalidated in the same way, not with --repair; every piece
and the reference need 6 to 225 frames), and every entry of "takes" gains "cos", the K cosines of the piece.
--repair [ROUNDS]: behind the sampler (and --takes) only the badly aligned words of every piece are spoken again, ROUNDS times
(default 1), and a repaired piece is kept where it scores strictly better (api.Repair; unvalidated on trained weights like --takes);
with --words the JSON gains "repair": [{piece, kept, bad, free, before, after}, ...], one list entry per round in each field.
--rate R / --encoding pcm16|mulaw|alaw: the joined waveform is resampled and encoded on the device (api.Delivery) and written as a WAV
of that format; not together with --words / --srt.
--watermark KEY [--watermark-strength S]: the joined waveform is marked with the key on the device (api.Watermark; 24000 Hz
PCM16 only, with and without --stream); python -m smalltts_amd.scripts.detect --wav out.wav --key KEY finds the mark again.
--stream: the WAV is written while the text is still being spoken (api.SmallTTS.synthesize_long_stream, audio.WavStreamWriter): one
chunk per group of pieces, the first after one piece's work; the time to the first chunk and the total are printed.  --batch-sizes
1,2,4,8 (the default ramp) or `none` (groups of --max-batch, the file --stream-less runs write, byte for byte).  --words / --srt /
--take are written at the end from what the chunks carried; the per-piece reports of --takes / --repair are not streamed.
--speed X / --fit-seconds S: the joined waveform is retimed on the device behind the join (api.Retime, DESIGN 8n: WSOLA, the pitch is
kept), X times as fast or to exactly S seconds; --words / --srt then count the retimed samples.  Not with --stream."""
import argparse
import json
import time
from pathlib import Path

import numpy as np

from ..api import SAMPLE_RATE, Endpointing, Repair, Retime, SmallTTS, Takes, estimate_duration, format_srt, save_take, split_text, token_groups
from ..audio import WavStreamWriter, read_wav
from ..phonemes import decode_token_ids, get_token_ids, parse_tokens_arg
from ._common import add_delivery_args, add_engine_args, add_watermark_args, delivery_for, pcm16_host, watermark_for, write_output


def group_texts(token_lists) -> list:
    """(piece index, kind, phonemes) of every token group of every piece, in text order: what word i of synthesize_long is."""
    return [(i, kind, ph) for i, toks in enumerate(token_lists) for kind, ph, _t0, _t1 in token_groups(toks)]


def words_json(words, texts, takes=None, repair=None, extra=None) -> str:
    """synthesize_long's words + group_texts -> the --words file: a JSON list of {index, piece, kind, phonemes, start, end (samples),
    start_s, end_s (seconds)}.  With `takes` (synthesize_long's return_takes) the file is {"words": that list, "takes": [{piece,
    winner, seed, totals}, ...]}, one entry per piece; a total that is not finite is written as null.  With `repair`
    (synthesize_long's return_repair) the file is such an object with "repair": [{piece, kept, bad, free, before, after}, ...], every
    field but `piece` a list with one entry per round."""
    if len(words) != len(texts):
        raise ValueError(f"{len(words)} timed groups for {len(texts)} groups of the text")
    rows = [{"index": int(gi), "piece": int(pi), "kind": kind, "phonemes": ph, "start": int(s), "end": int(e),
             "start_s": round(int(s) / SAMPLE_RATE, 4), "end_s": round(int(e) / SAMPLE_RATE, 4)}
            for (gi, kind, s, e), (pi, _k, ph) in zip(words, texts)]
    fin = lambda v: float(v) if float("-inf") < float(v) < float("inf") else None
    if takes is not None or repair is not None:
        rows = {"words": rows}
    if takes is not None:
        # (Takes(ctc > 0) reports the K values of nll too, Takes(sv > 0) the K cosines behind them: `extra` names what the tuples carry)
        names = list(extra) if extra is not None else (["nll"] if takes and len(takes[0]) > 4 else [])
        rows["takes"] = [{"piece": i, "winner": int(t[0]), "seed": int(t[1]), "totals": [fin(v) for v in t[2]],
                          **{n: [fin(v) for v in t[4 + j]] for j, n in enumerate(names)}}
                         for i, t in enumerate(takes)]
    if repair is not None:
        rows["repair"] = [{"piece": i, "kept": [int(v) for v in kept], "bad": [int(c[0]) for c in counts], "free": [int(c[1]) for c in counts],
                           "before": [fin(v) for v in before], "after": [fin(v) for v in after]}
                          for i, (kept, counts, before, after) in enumerate(repair)]
    return json.dumps(rows, ensure_ascii=False, indent=1)


def piece_cues(segments, piece_texts) -> list:
    """return_segments + one text per piece -> SubRip cues (start, end, text); a piece without speech gives none."""
    return [(off, off + n, txt) for (off, n, _start, _gain), txt in zip(segments, piece_texts) if n > 0]


def word_cues(words, texts) -> list:
    return [(s, e, ph) for (_gi, _kind, s, e), (_pi, _k, ph) in zip(words, texts)]


def stream_to_wav(tts, args, dv, voice, **kw):
    """--stream: synthesize_long_stream into args.out as the chunks arrive -> what synthesize_long would have returned for `kw`
    (the waveform is NOT kept: a (1, total samples) view of one zero stands in for its shape)."""
    timed, want_pieces = kw.pop("return_segments", False), kw.get("return_pieces", False)
    for k in ("return_takes", "return_repair"):
        kw.pop(k, None)
    segments, words, made, total = [], [], [], 0
    t0 = time.perf_counter()
    first = None
    with WavStreamWriter(args.out, 24_000 if dv is None else dv.rate, "pcm16" if dv is None else dv.encoding) as wav:
        for chunk in tts.synthesize_long_stream(voice, batch_sizes=args.batch_sizes, **kw):
            if first is None:
                first = time.perf_counter() - t0
            wav.write(pcm16_host(chunk.audio) if dv is None else chunk.audio)
            total += chunk.audio.shape[1]
            segments += chunk.segments
            words += chunk.words or []
            made += chunk.pieces or []
    print(f"first chunk after {0.0 if first is None else first:.3f}s, all of it after {time.perf_counter() - t0:.3f}s")
    audio = np.broadcast_to(np.zeros((), np.float32), (1, total))
    res = (audio,) + ((segments, words) if timed else ()) + ((made,) if want_pieces else ())
    return res if len(res) > 1 else audio


def parse_args(argv=None):
    """The command line -> its namespace (argument errors exit, as argparse does)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--wav", required=True, help="reference audio file (the voice)")
    ap.add_argument("--text-file", default=None, help="text to speak (any length)")
    ap.add_argument("--tokens-file", default=None, help="pre-split pieces: one comma-separated token list per line")
    ap.add_argument("--durations", default=None, help="seconds per piece of --tokens-file, comma-separated (one value: all pieces)")
    ap.add_argument("--out", default="out/longform.wav")
    ap.add_argument("--gap-ms", type=float, default=120.0, help="silence between pieces")
    ap.add_argument("--fade-ms", type=float, default=5.0, help="raised-cosine fade at both ends of every piece")
    ap.add_argument("--trim", action="store_true", help="join the pieces at the ends of their speech, not of their guessed durations")
    ap.add_argument("--level", type=float, default=None, metavar="DBFS", help="with --trim: bring every piece's speech to this RMS level")
    ap.add_argument("--words", default=None, metavar="OUT.json", help="write the time of every word / punctuation mark / [event] (133 ms resolution)")
    ap.add_argument("--srt", default=None, metavar="OUT.srt", help="write one subtitle cue per piece, and OUT.words.srt with one cue per word group")
    ap.add_argument("--take", default=None, metavar="OUT.npz", help="save the pieces and the join parameters (for scripts/respeak.py)")
    ap.add_argument("--takes", type=int, default=None, metavar="K", help=f"sample every piece K times (1..{Takes.MAX_K}) and keep the best-aligned take")
    ap.add_argument("--ctc", type=float, default=None, metavar="W",
                    help="with --takes: add W * CTC nll / tokens of the latent phoneme recogniser to every take's score (loads the recogniser)")
    ap.add_argument("--sv", type=float, default=None, metavar="W",
                    help="with --takes: add W * (1 - cosine with the reference voice) of the latent speaker verifier to every take's score "
                         "(loads the verifier)")
    ap.add_argument("--repair", type=int, nargs="?", const=1, default=None, metavar="ROUNDS",
                    help=f"speak only the badly aligned words of every piece again, ROUNDS times (1..{Repair.MAX_ROUNDS}, default 1)")
    ap.add_argument("--max-batch", type=int, default=8)
    ap.add_argument("--in-flight", type=int, default=3)
    ap.add_argument("--stream", action="store_true", help="write the WAV chunk by chunk while the text is being spoken")
    ap.add_argument("--batch-sizes", default=None, metavar="N,N,...|none",
                    help="with --stream: pieces per group, the last value repeated (default 1,2,4,8); none = groups of --max-batch")
    ap.add_argument("--speed", type=float, default=None, metavar="X", help="retime the joined waveform: X times as fast, the pitch kept")
    ap.add_argument("--fit-seconds", type=float, default=None, metavar="S", help="retime the joined waveform to exactly S seconds")
    add_engine_args(ap)
    add_delivery_args(ap)
    add_watermark_args(ap)
    args = ap.parse_args(argv)
    if args.speed is not None and args.fit_seconds is not None:
        ap.error("--speed and --fit-seconds exclude each other")
    if (args.speed is not None or args.fit_seconds is not None) and args.stream:
        ap.error("--speed / --fit-seconds do not go with --stream (a retiming is not streamed)")
    try:
        args.retime = None if args.speed is None and args.fit_seconds is None else Retime(speed=args.speed, duration=args.fit_seconds)
    except ValueError as e:
        ap.error(str(e))
    args.mark, args.delivery = watermark_for(ap, args, delivery_for(args))   # --watermark: the joined waveform is marked on the device
    if args.batch_sizes is not None and not args.stream:
        ap.error("--batch-sizes needs --stream")
    if args.batch_sizes is not None and args.batch_sizes.strip().lower() != "none":
        try:
            args.batch_sizes = tuple(int(v) for v in args.batch_sizes.replace(",", " ").split())
        except ValueError:
            ap.error("--batch-sizes takes positive integers, comma-separated, or none")
        if not args.batch_sizes or min(args.batch_sizes) < 1:
            ap.error("--batch-sizes takes positive integers, comma-separated, or none")
    elif args.stream:
        args.batch_sizes = (1, 2, 4, 8) if args.batch_sizes is None else None
    if (args.rate is not None or args.encoding is not None) and (args.words or args.srt):
        ap.error("--rate / --encoding do not go with --words / --srt (their files count 24 kHz samples)")
    if (args.text_file is None) == (args.tokens_file is None):
        ap.error("pass either --text-file or --tokens-file")
    if args.tokens_file and not args.durations:
        ap.error("--tokens-file needs --durations")
    if args.level is not None and not args.trim:
        ap.error("--level needs --trim")
    if args.takes is not None and not 1 <= args.takes <= Takes.MAX_K:
        ap.error(f"--takes must lie in [1, {Takes.MAX_K}]")
    if args.repair is not None and not 1 <= args.repair <= Repair.MAX_ROUNDS:
        ap.error(f"--repair must lie in [1, {Repair.MAX_ROUNDS}]")
    if args.ctc is not None and (args.takes is None or not args.ctc >= 0.0 or args.ctc == float("inf")):
        ap.error("--ctc takes a finite weight >= 0 and needs --takes")
    if args.ctc and args.repair is not None:
        ap.error("--ctc and --repair exclude each other (repair's keep rule scores without the CTC term)")
    if args.sv is not None and (args.takes is None or not args.sv >= 0.0 or args.sv == float("inf")):
        ap.error("--sv takes a finite weight >= 0 and needs --takes")
    if args.sv and args.repair is not None:
        ap.error("--sv and --repair exclude each other (repair's keep rule scores without the speaker term)")
    if args.takes is not None and args.takes * args.max_batch > Takes.MAX_ROWS:
        args.max_batch = Takes.MAX_ROWS // args.takes   # synthesize_long's rule, applied here so that --take records the group size used
    return args


def main(argv=None):
    args = parse_args(argv)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    print("loading")
    tts = SmallTTS(weights=args.weights, device=args.device, precision=args.precision, num_steps=args.steps, seed=args.seed,
                   recogniser=bool(args.ctc), verifier=bool(args.sv))
    print("encoding reference audio")
    y, sr = read_wav(args.wav)
    if y.ndim == 2:
        y = y.mean(axis=1)
    voice = tts.encode_voice_wav(y, sr)
    kw = dict(seed=args.seed, gap_ms=args.gap_ms, fade_ms=args.fade_ms, max_batch=args.max_batch, in_flight=args.in_flight,
              trim=Endpointing(level_dbfs=args.level) if args.trim else None)
    dv = args.delivery
    if dv is not None:
        kw.update(deliver=dv)                              # the joined waveform leaves the device at that rate and encoding
    if args.mark is not None:
        kw.update(watermark=args.mark)
    if args.retime is not None:
        kw.update(retime=args.retime)                      # behind the join, in front of the mark and the delivery
    timed = bool(args.words or args.srt)
    if timed:
        kw.update(return_segments=True, return_words=True)
    if args.take:
        kw.update(return_pieces=True)
    if args.takes is not None:
        kw.update(takes=Takes(args.takes, ctc=args.ctc or 0.0, sv=args.sv or 0.0) if (args.ctc or args.sv) else args.takes, return_takes=True)
    if args.repair is not None:
        kw.update(repair=args.repair, return_repair=True)
    speak = tts.synthesize_long if not args.stream else (lambda *a, **k: stream_to_wav(tts, args, dv, *a, **k))
    if args.tokens_file:
        with open(args.tokens_file) as f:
            token_lists = [parse_tokens_arg(line) for line in f if line.strip()]
        durs = [float(d) for d in args.durations.replace(",", " ").split()]
        if len(durs) == 1:
            durs = durs * len(token_lists)
        print(f"generating {len(token_lists)} pieces")
        piece_texts = [decode_token_ids(t) for t in token_lists]
        audio = speak(voice, token_lists=token_lists, durations=durs, **kw)
    else:
        with open(args.text_file) as f:
            text = f.read()
        tok = lambda t: get_token_ids(t, backend=args.tokenizer)
        pieces = split_text(text, count_tokens=lambda t: len(tok(t)))
        print(f"generating {len(pieces)} pieces")
        token_lists, piece_texts = [tok(p) for p in pieces], pieces
        audio = speak(voice, token_lists=token_lists, durations=[estimate_duration(p) for p in pieces], **kw)
    chosen = mended = None
    if args.stream:
        args.takes = args.repair = None                    # (their reports are not streamed)
    if args.repair is not None:                            # (the very last element)
        audio, mended = (audio[:-1] if len(audio) > 2 else audio[0]), audio[-1]
        print("repaired: " + " ".join(str(int(sum(kept))) for kept, _counts, _before, _after in mended))
    if args.takes is not None:
        audio, chosen = (audio[:-1] if len(audio) > 2 else audio[0]), audio[-1]
        print("takes kept: " + " ".join(str(t[0]) for t in chosen))
    if args.take:
        audio, taken = (audio[:-1] if timed else audio[0]), audio[-1]
        Path(args.take).parent.mkdir(parents=True, exist_ok=True)
        save_take(args.take, taken, gap_ms=args.gap_ms, fade_ms=args.fade_ms, max_batch=args.max_batch, in_flight=args.in_flight,
                  trim=args.trim, level_dbfs=args.level)
        print(f"{args.take} ({len(taken)} pieces)")
    if timed:
        audio, segments, words = audio
        texts = group_texts(token_lists)
        if args.words:
            Path(args.words).parent.mkdir(parents=True, exist_ok=True)
            Path(args.words).write_text(words_json(words, texts, chosen, mended, (["nll"] if args.ctc else []) + (["cos"] if args.sv else [])), encoding="utf-8")
            print(f"{args.words} ({len(words)} word groups)")
        if args.srt:
            Path(args.srt).parent.mkdir(parents=True, exist_ok=True)
            Path(args.srt).write_text(format_srt(piece_cues(segments, piece_texts)), encoding="utf-8")
            wpath = str(Path(args.srt).with_suffix("")) + ".words.srt"
            Path(wpath).write_text(format_srt(word_cues(words, texts)), encoding="utf-8")
            print(f"{args.srt}, {wpath}")
    if not args.stream:                                    # (streamed: the file is complete already)
        write_output(args.out, audio.squeeze(0), dv)
    print(f"{args.out} ({audio.shape[1] / (24_000 if dv is None else dv.rate):.1f}s)")


if __name__ == "__main__":
    main()
