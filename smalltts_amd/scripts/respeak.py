"""python -m smalltts_amd.scripts.respeak --take T.npz --wav ref.wav --piece I (--frames A:B | --groups A:B) [--seed S]
    [--start-step K] [--takes K [--ctc W] [--sv W]] --out out.wav [--take-out T2.npz]
Speaks a span of one piece of a long take again and keeps everything else: the take (scripts/longform.py --take) holds every piece's
tokens and latents; frames [A, B) of piece I, or the frames its token groups [A, B) touch (the spans longform --words saved), are
regenerated with the rest of the piece pinned (api.SmallTTS.respeak), the whole take is rendered again with its own join parameters
(api.SmallTTS.render_long) and written out, with the updated take next to it.  A new take needs a new --seed (none: one is drawn).
--tokens: the piece's new token list when the text changes (the take's prefix is prepended); --new-frames: the length of the
regenerated region.  --takes K: the span is re-spoken K times, every take with the same pins, and the best-aligned one is kept
(api.Takes; the updated take records the winner's seed).  Only the mechanism is verified: how well the 4-step student inpaints, and
what the takes' score is worth, are unvalidated on trained weights.  --ctc W: the takes' score gains W * CTC nll / tokens of the latent
phoneme recogniser (api.Takes(ctc=); loads the recogniser; unvalidated in the same way).  --sv W: it gains W * (1 - cosine)
of every take's speaker embedding with the reference voice's (api.Takes(sv=); loads the latent speaker verifier; unvalidated
in the same way; the piece and the reference need 6 to 225 frames)."""
import argparse
from pathlib import Path

from ..api import Endpointing, Piece, SmallTTS, Takes, frames_of_groups, load_take, save_take, token_groups
from ..audio import read_wav, write_wav_pcm16
from ..phonemes import parse_tokens_arg
from ._common import add_engine_args


def parse_range(text: str, what: str):
    """'A:B' -> (A, B) with A < B."""
    try:
        a, b = (int(v) for v in text.split(":"))
    except ValueError:
        raise ValueError(f"{what} must be A:B, two integers, got {text!r}") from None
    if not 0 <= a < b:
        raise ValueError(f"{what}: need 0 <= A < B, got {a}:{b}")
    return a, b


def span_frames(piece: Piece, frames=None, groups=None):
    """The frames to regenerate in `piece`: --frames as given, --groups through the piece's saved token spans."""
    if (frames is None) == (groups is None):
        raise ValueError("pass either --frames or --groups")
    if frames is not None:
        f0, f1 = parse_range(frames, "--frames")
        if f1 > piece.latents.shape[0]:
            raise ValueError(f"--frames {f0}:{f1} outside the piece's {piece.latents.shape[0]} frames")
        return f0, f1
    if piece.spans is None:
        raise ValueError("--groups needs the token spans of the piece: make the take with longform --words")
    g0, g1 = parse_range(groups, "--groups")
    return frames_of_groups(token_groups(piece.tokens[piece.prefix_len:]), piece.spans, g0, g1, token0=piece.prefix_len)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--take", required=True, help="the take to change (longform --take)")
    ap.add_argument("--wav", required=True, help="reference audio file (the voice the take was spoken in)")
    ap.add_argument("--piece", type=int, required=True, help="index of the piece")
    ap.add_argument("--frames", default=None, metavar="A:B", help="regenerate frames [A, B) of the piece (one frame = 3200 samples)")
    ap.add_argument("--groups", default=None, metavar="A:B", help="regenerate the frames of the piece's token groups [A, B)")
    ap.add_argument("--new-frames", type=int, default=None, help="length of the regenerated region (default: B - A frames)")
    ap.add_argument("--start-step", type=int, default=0, help="run only the sampler steps from K on, from the take's latents")
    ap.add_argument("--takes", type=int, default=None, metavar="K", help=f"re-speak the span K times (1..{Takes.MAX_K}) and keep the best-aligned take")
    ap.add_argument("--ctc", type=float, default=None, metavar="W",
                    help="with --takes: add W * CTC nll / tokens of the latent phoneme recogniser to every take's score (loads the recogniser)")
    ap.add_argument("--sv", type=float, default=None, metavar="W",
                    help="with --takes: add W * (1 - cosine with the reference voice) of the latent speaker verifier to every take's score "
                         "(loads the verifier)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--take-out", default=None, metavar="T2.npz", help="where the updated take goes (default: next to --out)")
    add_engine_args(ap)
    args = ap.parse_args(argv)
    pieces, join = load_take(args.take)
    if not 0 <= args.piece < len(pieces):
        ap.error(f"--piece must lie in [0, {len(pieces)})")
    if args.takes is not None and not 1 <= args.takes <= Takes.MAX_K:
        ap.error(f"--takes must lie in [1, {Takes.MAX_K}]")
    if args.ctc is not None and (args.takes is None or not args.ctc >= 0.0 or args.ctc == float("inf")):
        ap.error("--ctc takes a finite weight >= 0 and needs --takes")
    if args.sv is not None and (args.takes is None or not args.sv >= 0.0 or args.sv == float("inf")):
        ap.error("--sv takes a finite weight >= 0 and needs --takes")
    old = pieces[args.piece]
    try:
        f0, f1 = span_frames(old, args.frames, args.groups)
    except ValueError as e:
        ap.error(str(e))
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    print("loading")
    tts = SmallTTS(weights=args.weights, device=args.device, precision=args.precision, num_steps=args.steps, seed=args.seed,
                   recogniser=bool(args.ctc), verifier=bool(args.sv))
    print("encoding reference audio")
    y, sr = read_wav(args.wav)
    if y.ndim == 2:
        y = y.mean(axis=1)
    voice = tts.encode_voice_wav(y, sr)
    seed = tts._next_seed() if args.seed is None else int(args.seed)
    tokens = list(old.tokens)
    if args.tokens:
        tokens = tokens[:old.prefix_len] + parse_tokens_arg(args.tokens)
    timed = old.spans is not None
    print(f"re-speaking frames [{f0}, {f1}) of piece {args.piece} (seed {seed})")
    res = tts.respeak(old.tokens, old.latents, (f0, f1), voice=voice, new_tokens=tokens, new_frames=args.new_frames, seed=seed,
                      start_step=args.start_step, prefix_len=old.prefix_len,
                      **({"align": True, "return_alignment": True} if timed else {}),
                      **({} if args.takes is None else {"takes": Takes(args.takes, ctc=args.ctc or 0.0, sv=args.sv or 0.0) if (args.ctc or args.sv) else args.takes,
                                                       "return_takes": True}))
    if args.takes is not None:
        winner, seed = res[-1][0], res[-1][1]
        print(f"take {winner} of {args.takes} kept (seed {seed})")
    pieces[args.piece] = Piece(tokens, old.prefix_len, res[1], seed, res[3][1] if timed else None)
    trim = Endpointing(level_dbfs=join["level_dbfs"]) if join["trim"] else None
    audio = tts.render_long(pieces, gap_ms=join["gap_ms"], fade_ms=join["fade_ms"], max_batch=join["max_batch"],
                            in_flight=join["in_flight"], trim=trim)
    write_wav_pcm16(args.out, audio.squeeze(0), 24_000)
    print(f"{args.out} ({audio.shape[1] / 24_000:.1f}s)")
    take_out = args.take_out or str(Path(args.out).with_suffix(".npz"))
    Path(take_out).parent.mkdir(parents=True, exist_ok=True)
    save_take(take_out, pieces, **join)
    print(f"{take_out} ({len(pieces)} pieces)")


if __name__ == "__main__":
    main()
