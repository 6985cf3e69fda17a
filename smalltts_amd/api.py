"""Drop-in Python API of the reference (`smalltts.SmallTTS`, `estimate_duration`, codec `Encoder` /
`Decoder`) on top of the gfx950 engine.

Mirrors reference `src/smalltts/infer/onnx.py` (class SmallTTS :50-159, constants :11-14,
estimate_duration :17-18) and `src/smalltts/codec/onnx.py` (Encoder/Decoder :34-75): same positional
arguments, argument meaning, return types and error-by-exception behaviour.  The three ONNX path
arguments are accepted for call compatibility; weights come from `weights=` (keyword-only
addition): a flat weight file written by `smalltts_amd.weights.save_weight_file`, a torch
checkpoint holding the reference's state_dict (optionally under "student_model",
distill.py:468-479), or "synthetic:<seed>" (seeded random weights — there are no released weights
offline).  Unlike the reference, `forward` runs all utterances as ONE padded batch on the GPU.
"""
from __future__ import annotations

import collections
import contextlib
import hashlib
import os
from typing import Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .engine import (ASR_LONG_MAX_FRAMES, ASR_MAX_ROWS, ASR_UPSAMPLE, CTC_LONG_MAX_TOKENS, DEFAULT_PRECISION, SITES, SV_DIM, SV_MAX_ROWS,
                     SV_MIN_FRAMES, HipEngine)
from .weights import DEFAULT_CODEC, CodecSpec, all_param_specs, asr_param_specs, load_weight_file, sv_param_specs
# the option records (options.py) and the host arithmetic (plans.py) live in modules of their own; every name stays importable from here
from .options import (ALIGN_MAX_FRAMES, ALIGN_MAX_TOKENS, TAKE_JOIN_KEYS, Alignment, Delivery, Endpointing, Piece, Pitch, Repair, Retime,
                      Takes, Watermark, _Frozen, as_alignment, as_delivery, as_endpointing, as_pitch, as_repair, as_retime, as_takes,
                      as_watermark, load_take, marked_delivery, save_take)
from .plans import (CHARS_PER_SECOND, CTC_HOP, HOP_SIZE, NUM_STEPS, SAMPLE_RATE, _CLAUSE_END, _SENTENCE_END, _check_pins,
                    _default_count_tokens, _frames, _hard_cut, _srt_time, _units, codec_spans, estimate_duration, fade_table,
                    format_srt, frames_of_groups, group_confidence, long_windows, phoneme_error_rate, piece_seed, pitch_f0,
                    pitch_rows, pitch_word_stats, plan_long, plan_packed, repair_seed, retime_anchors, retime_rows, retime_times,
                    speaking_rate, splice_pins, split_text, stream_chunks, stream_groups, take_seed, token_groups, word_times)

PITCH_MAX_WORKSPACE = 256 << 20   # SmallTTS.pitch: rows ride in groups whose workspace stays below this


class PitchTrack(NamedTuple):
    """What SmallTTS.pitch returns: `f0` in Hz per frame (float64, 0 where unvoiced), `strength` (fp32, the score at the chosen lag, 0
    where unvoiced); frame f starts at sample f * `hop` of the `sr` Hz audio."""
    f0: np.ndarray
    strength: np.ndarray
    hop: int
    sr: int


def _pitch_device(eng: HipEngine, y: torch.Tensor, pt: "Pitch", max_row: Optional[int] = None):
    """y: 24 kHz samples, 1-d fp32 on the device -> (lag (F,) int32, peak (F, 3) fp32) on the host, F = ceil(n / hop)."""
    n = int(y.numel())
    rows = pitch_rows(n, pt.hop) if max_row is None else pitch_rows(n, pt.hop, max_row=max_row)
    F = -(-n // pt.hop)
    lag, peak = np.zeros((F,), np.int32), np.zeros((F, 3), np.float32)
    per_row = int(eng.lib.smtts_pitch_workspace_bytes(eng.h, 1, max(r[1] for r in rows), pt.hop, pt.lmin, pt.lmax))
    if per_row <= 0:
        raise ValueError(f"pitch: {eng.lib.smtts_last_error(eng.h).decode()}")
    group = max(1, min(1024, PITCH_MAX_WORKSPACE // per_row))
    for g0 in range(0, len(rows), group):
        grp = rows[g0: g0 + group]
        if len(grp) == 1:
            batch = y[grp[0][0]: grp[0][0] + grp[0][1]].reshape(1, 1, -1).contiguous()
        else:
            batch = torch.zeros(len(grp), 1, max(r[1] for r in grp), device=eng.device)
            for b, (s0, sn, _f0, _fn) in enumerate(grp):
                batch[b, 0, :sn] = y[s0: s0 + sn]
        lg, pk = eng.pitch(batch, [r[1] for r in grp], pt)
        lg, pk = lg.cpu().numpy(), pk.cpu().numpy()
        for b, (s0, _sn, f0, fn) in enumerate(grp):
            k = f0 - s0 // pt.hop                              # the row's own index of the first frame it keeps
            lag[f0: f0 + fn], peak[f0: f0 + fn] = lg[b, k: k + fn], pk[b, k: k + fn]
    return lag, peak


def pitch_track(engine: HipEngine, audio, pitch=None, words=None):
    """The F0 track of 24 kHz mono audio of any length (engine.pitch: NCCF scores and a Viterbi path on the device) ->
    PitchTrack(f0, strength, hop, sr), one entry per frame of `hop` samples, ceil(n / hop) of them (audio: an array, or a tensor on
    any device; one on the engine's device is not copied); with `words` (align_words' or
    align_wav's rows) -> (the track, [(row, dict(f0_median, f0_min, f0_max, voiced)), ...]) by plans.pitch_word_stats.  `pitch`: a
    Pitch, None for its defaults.  Audio longer than 30 s is cut into rows that share 1 s with their neighbours (plans.pitch_rows);
    the rows ride in groups whose workspace stays below 256 MiB.  Needs no weights: any HipEngine will do.  The constants were
    checked on synthetic signals only: nothing is claimed about accuracy on speech."""
    pt = as_pitch(pitch)
    a = audio.detach() if isinstance(audio, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(audio), np.float32))
    if (a.dim() != 1 and not (a.dim() == 2 and 1 in a.shape)) or a.numel() < 1:
        raise ValueError(f"pitch: mono audio of at least one sample, got an array of shape {tuple(a.shape)}")
    # a tensor that already lies on the engine's device (pitch_track_wav's resampled audio) is tracked where it is
    lag, peak = _pitch_device(engine, a.reshape(-1).to(device=engine.device, dtype=torch.float32).contiguous(), pt)
    f0, strength = pitch_f0(lag, peak, SAMPLE_RATE)
    track = PitchTrack(f0, strength, pt.hop, SAMPLE_RATE)
    if words is None:
        return track
    words = list(words)
    return track, list(zip(words, pitch_word_stats(words, f0, pt.hop)))


def pitch_track_wav(engine: HipEngine, audio, sr: int, pitch=None, words=None):
    """pitch_track of a recording: mono samples at `sr` Hz are resampled to 24 kHz on the device first, as align_wav does; `words`
    then count 24 kHz samples, as the aligners' rows do."""
    a = np.asarray(audio, np.float32)
    if a.ndim != 1 and not (a.ndim == 2 and 1 in a.shape):
        raise ValueError(f"pitch_wav: a mono recording, got an array of shape {a.shape}")
    sr = int(sr)
    if sr < 1 or a.size < 1:
        raise ValueError(f"pitch_wav: at least one sample at a positive rate, got {a.size} samples at {sr} Hz")
    y = engine.resample(a.reshape(-1), sr, SAMPLE_RATE)
    return pitch_track(engine, y.reshape(-1), pitch, words)


DEFAULT_WEIGHTS = os.environ.get("SMALLTTS_WEIGHTS", "assets/smalltts.smtts")

_ENGINES: Dict[tuple, HipEngine] = {}


def _piece_latents(pieces) -> List[np.ndarray]:
    """render_long's input: Pieces or (n_i, 64) arrays -> fp32 arrays."""
    out = []
    for i, p in enumerate(pieces):
        lat = np.asarray(p.latents if isinstance(p, Piece) else p, np.float32)
        if lat.ndim != 2 or lat.shape[1] != 64 or lat.shape[0] < 1:
            raise ValueError(f"render_long: piece {i} must hold (n, 64) latents with n >= 1, got {lat.shape}")
        out.append(lat)
    return out


def _split_sources(weights) -> List[str]:
    if isinstance(weights, (list, tuple)):
        return [str(w) for w in weights]
    return [w for w in str(weights).split("+") if w]


def _validated(tensors: Dict[str, object], source: str, codec: CodecSpec) -> Dict[str, object]:
    """Reject a tensor whose shape is not the inventory's BEFORE it reaches the packers: the kernels assume the model's
    strides (960 / 2400 / 512 ...), so a checkpoint of another model size must be a clean error naming the tensor."""
    want = dict(all_param_specs(codec) + asr_param_specs() + sv_param_specs())
    bad = [(k, tuple(v.shape), want[k]) for k, v in tensors.items() if k in want and tuple(v.shape) != tuple(want[k])]
    if bad:
        k, got, exp = bad[0]
        raise ValueError(f"{source}: tensor {k!r} has shape {got}, this build expects {exp} "
                         f"({len(bad)} mismatching tensor{'s' if len(bad) > 1 else ''}) — not a DiTModel(64) / CodecSpec checkpoint")
    unknown = [k for k in tensors if k not in want]
    if unknown and len(unknown) == len(tensors):
        raise ValueError(f"{source}: none of its {len(tensors)} tensors is a parameter of this build (first: {unknown[0]!r})")
    # A codec.* tensor the engine WOULD apply (biases, layer scales and the final norm are optional at run time) but that the
    # CodecSpec in force says is absent must not vanish silently: the audio would come out wrong with no error.
    full = dict(all_param_specs(CodecSpec(**{**codec.to_dict(), "conv_bias": True, "ffn_bias": True, "layer_scale": True, "final_norm": True})))
    dropped = [k for k in unknown if k in full]
    if dropped:
        raise ValueError(f"{source}: tensor {dropped[0]!r} (+{len(dropped) - 1} more) is an optional codec parameter that this "
                         "CodecSpec switches off (conv_bias / ffn_bias / layer_scale / final_norm) — it would be ignored; "
                         "load it with the matching spec (convert.py --codec-spec, or a .smtts file that carries its spec)")
    return {k: v for k, v in tensors.items() if k in want}


def _load_weights_into(eng: HipEngine, weights, parts: Sequence[str]) -> None:
    """`weights`: one source or several joined with '+' (or a list), applied in order:
      * ``*.pt / *.pth / *.ckpt``  torch checkpoint holding the reference's ``DiTModel`` state_dict, bare or under
        ``"student_model"`` / ``"model"`` with the wrapper prefixes of distill.py:47-54 (codec.* keys are taken too);
      * any other path             flat weight file (`weights.save_weight_file`, written by `smalltts_amd.convert`);
      * ``synthetic[:seed]``       seeded random weights for every requested part NOT provided by an earlier source.
    e.g. ``"dmd.pt+codec.smtts"`` (DiT checkpoint + separately converted codec) or ``"dmd.pt+synthetic:7"``."""
    have: set = set()
    prefixes = {"dit": ("velocity.",), "decoder": ("codec.decoder.",), "encoder": ("codec.encoder.",), "asr": ("asr.",), "sv": ("sv.",)}
    codec = eng.codec_spec

    def note(names):
        for part, pre in prefixes.items():
            if any(n.startswith(pre) for n in names):
                have.add(part)

    for src in _split_sources(weights):
        if src.startswith("synthetic"):
            seed = int(src.split(":", 1)[1]) if ":" in src else 0
            todo = [p for p in parts if p not in have]
            if todo:
                eng.load_synthetic(seed, parts=todo)
                have.update(todo)
            continue
        if not os.path.exists(src):
            raise FileNotFoundError(
                f"weight file {src!r} not found. The reference downloads its ONNX weights from HuggingFace "
                "(assets/ensure.py); offline, pass weights='synthetic:<seed>' or a converted weight file.")
        if src.endswith((".pt", ".pth", ".ckpt")):
            from .convert import state_dict_from_checkpoint
            tensors = state_dict_from_checkpoint(torch.load(src, map_location="cpu", weights_only=True))
        else:
            tensors, cdict = load_weight_file(src)
            if cdict:
                codec = CodecSpec(**cdict)
                eng.set_codec_spec(codec)
        tensors = _validated(tensors, src, codec)
        eng.load_state_dict(tensors)
        note(tensors)
    eng.finalize()
    # real weights (anything but the seeded recipe): hold the preset to split-bf16 on a probe batch once, demote what drifts
    if any(not src.startswith("synthetic") for src in _split_sources(weights)) and os.environ.get("SMTTS_CALIBRATE", "1") != "0":
        eng.calibrate()


def get_engine(weights: Optional[str] = None, device: int = 0, precision: str = DEFAULT_PRECISION,
               parts: Sequence[str] = ("dit", "decoder", "encoder")) -> HipEngine:
    """One engine (one weight copy) per (weights, device, parts); shared by SmallTTS/Encoder/Decoder.  parts: of "dit", "decoder",
    "encoder", "asr" (the latent phoneme recogniser) and "sv" (the latent speaker verifier); the last two are
    optional and not among the defaults."""
    unknown = [p for p in parts if p not in ("dit", "decoder", "encoder", "asr", "sv")]
    if unknown:
        raise ValueError(f"get_engine: unknown part {unknown[0]!r} (dit, decoder, encoder, asr, sv)")
    weights = weights or DEFAULT_WEIGHTS
    key = ("+".join(_split_sources(weights)), int(device), tuple(sorted(parts)))
    eng = _ENGINES.get(key)
    if eng is None:
        eng = HipEngine(device, precision)
        _load_weights_into(eng, weights, parts)
        _ENGINES[key] = eng
    if eng.precision != precision:
        eng.set_precision(precision)
    return eng


_NP_OF = {torch.float32: np.float32, torch.int64: np.int64, torch.int32: np.int32, torch.int16: np.int16, torch.uint8: np.uint8}


class LongChunk(NamedTuple):
    """One chunk of synthesize_long_stream: the next `audio.shape[1]` samples of the joined waveform, what one group of pieces added."""
    audio: np.ndarray                    # (1, s_g), in the dtype synthesize_long would return
    index: int                           # the group's number, from 0
    offset: int                          # the chunk's first sample in the joined stream (in output samples with deliver=)
    segments: List[tuple]                # this chunk's pieces: (offset in the stream, n, start inside the piece, gain), as synthesize_long's
    words: Optional[List[tuple]]         # return_words: (group index, kind, start sample, end sample) of this chunk's pieces, else None
    pieces: Optional[List["Piece"]]      # return_pieces: this chunk's Pieces, else None


class _LongRequest(NamedTuple):
    """What SmallTTS._long_request makes of the arguments synthesize_long and synthesize_long_stream share."""
    wm: Optional["Watermark"]
    dv: Optional["Delivery"]
    ep: Optional["Endpointing"]
    al: Optional["Alignment"]
    tk: Optional["Takes"]                # None also for one take with nothing to report
    rp: Optional["Repair"]
    K: int
    prefix: List[int]                    # the prepended transcription's tokens
    toks: List[List[int]]                # every piece's tokens, the prefix in front
    ns: List[int]                        # frames per piece
    max_batch: int                       # lowered to 64 // K where K * max_batch would pass the sampler's rows


class Voice(_Frozen):
    """A reference voice encoded once: the reference half of the cross-KV cache, `k_ref` / `v_ref` (12, 1, 8, R, 120) fp32 on the
    engine's device (what cond_encode returns for this reference at B = 1), its length `R` and the `engine` it belongs to.
    `speaker`: the reference's speaker embedding, a (192,) fp32 tensor on the device (engine.sv_embed of the reference latents;
    DESIGN 8j), or None: the engine held no verifier part when the voice was encoded, or the reference is under 6 or over 225 frames.
    Immutable; any number of calls (and batches in flight) of that engine may read it."""
    __slots__ = ("engine", "k_ref", "v_ref", "R", "speaker")

    def __init__(self, engine: HipEngine, k_ref: torch.Tensor, v_ref: torch.Tensor, speaker: Optional[torch.Tensor] = None) -> None:
        self._set(engine=engine, k_ref=k_ref, v_ref=v_ref, R=int(k_ref.shape[3]), speaker=speaker)


class _Batch(NamedTuple):
    """One batch on the device, enqueued on the stream that was current when it was made; nothing here has been read back.
    `rerun()` enqueues the same work again on the current stream (the fp16 range guard's second pass), the tap, the path and the
    endpoints included when the record has them, and returns a new record; its closure keeps the batch's voices alive.  With takes=
    the rows are the winners: latents, mass and spans are those of the take kept for each row."""
    audio: torch.Tensor                  # (B, 1, HOP_SIZE * Nmax) fp32; causal decoder => row b is its first HOP_SIZE * ns[b] samples
    latents: torch.Tensor                # (B, Nmax, 64) fp32
    mass: Optional[torch.Tensor]         # align=: the tapped text attention (engine.sample), else None
    spans: Optional[torch.Tensor]        # align=: (B, P, 2) (first, last) frame per token (engine.align_path), else None
    seg: Optional[torch.Tensor]          # endpoints: (B, 2) int64 (start, n) per row (engine.endpoints), else None
    gain: Optional[torch.Tensor]         # endpoints: (B,) fp32, else None
    ns: List[int]                        # frames per row
    rerun: Callable[[], "_Batch"]
    winner: Optional[torch.Tensor] = None  # takes=: (B,) int32, the take kept per row (engine.take_select); None with one take
    total: Optional[torch.Tensor] = None   # takes=: (B * K,) fp32, every take's total, piece-major (engine.take_scores), else None
    feat: Optional[torch.Tensor] = None    # takes=: (B * K, 4) int32 (cells, skipped, longest, idle), else None
    nll: Optional[torch.Tensor] = None     # Takes(ctc > 0): (B * K,) fp32, every take's CTC nll, piece-major (engine.ctc_score), else None
    cos: Optional[torch.Tensor] = None     # Takes(sv > 0): (B * K,) fp32, every take's cosine with its reference voice (engine.sv_cosine), else None
    rp_kept: Optional[List[torch.Tensor]] = None     # repair=: per round (B,) int32, 1 where the repaired row was kept (engine.repair_keep)
    rp_counts: Optional[List[torch.Tensor]] = None   # repair=: per round (B, 2) int32 (bad tokens, freed frames) (engine.repair_plan)
    rp_totals: Optional[List[torch.Tensor]] = None   # repair=: rounds + 1 (B,) fp32: the rows' totals before round 1 and after every round


def _read_takes(recs: Sequence[_Batch], K: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """What takes= left in finished batches, in ONE small read-back: -> (winner (n,) int32, totals (n, K) fp32, features (n, K, 4)
    int32) over the rows of all records in order; a record without a winner table (one take) reports 0."""
    parts = []
    for rec in recs:
        parts += [rec.total.view(torch.int32), rec.feat.reshape(-1)] + ([] if rec.winner is None else [rec.winner])
    flat = torch.cat(parts).cpu().numpy()
    wins, tots, feats, pos = [], [], [], 0
    for rec in recs:
        R = int(rec.total.shape[0])
        G = R // K
        tots.append(flat[pos: pos + R].view(np.float32).reshape(G, K))
        feats.append(flat[pos + R: pos + 5 * R].reshape(G, K, 4))
        pos += 5 * R
        if rec.winner is None:
            wins.append(np.zeros(G, np.int32))
        else:
            wins.append(flat[pos: pos + G])
            pos += G
    return np.concatenate(wins), np.concatenate(tots), np.concatenate(feats)


def _read_nll(recs: Sequence[_Batch], K: int) -> np.ndarray:
    """The CTC term of Takes(ctc > 0) of finished batches, in one small read-back: -> nll (n, K) fp32 over the rows of all records."""
    return torch.cat([rec.nll for rec in recs]).cpu().numpy().reshape(-1, K)


def check_takes_ctc(what: str, tk: Optional["Takes"], rp: Optional["Repair"], eng: HipEngine) -> bool:
    """Takes(ctc > 0) asks for the recogniser part and excludes repair= (its keep rule re-scores with take_scores alone).  -> whether the
    CTC term is on."""
    if tk is None or tk.ctc == 0.0:
        return False
    if rp is not None:
        raise ValueError(f"{what}: Takes(ctc > 0) and repair= exclude each other (repair's keep rule scores without the CTC term)")
    if not eng.has("asr"):
        raise ValueError(f"{what}: Takes(ctc > 0) needs the recogniser part (SmallTTS(recogniser=True) or get_engine(parts=(..., 'asr')))")
    return True


def _read_cos(recs: Sequence[_Batch], K: int) -> np.ndarray:
    """The speaker term of Takes(sv > 0) of finished batches, in one small read-back: -> cos (n, K) fp32 over the rows of all records."""
    return torch.cat([rec.cos for rec in recs]).cpu().numpy().reshape(-1, K)


def _takes_extra(recs: Sequence[_Batch], K: int, n: int) -> List[tuple]:
    """What return_takes appends to every row's tuple: nll (K,) with Takes(ctc > 0), then cos (K,) with Takes(sv > 0)."""
    extra = [()] * n
    if recs[0].nll is not None:
        extra = [e + (v,) for e, v in zip(extra, _read_nll(recs, K))]
    if recs[0].cos is not None:
        extra = [e + (v,) for e, v in zip(extra, _read_cos(recs, K))]
    return extra


def check_takes_sv(what: str, tk: Optional["Takes"], rp: Optional["Repair"], eng: HipEngine, ns: Optional[Sequence[int]] = None,
                   voices: Optional[Sequence["Voice"]] = None, rs: Optional[Sequence[int]] = None) -> bool:
    """Takes(sv > 0) asks for the verifier part, excludes repair= (its keep rule re-scores with take_scores alone), and needs 6 to 225
    frames in every row (`ns`) and an embedding for every reference: the `speaker` of every Voice, or 6 to 225 reference frames
    (`rs`).  Everything is checked in front of any launch.  -> whether the speaker term is on."""
    if tk is None or tk.sv == 0.0:
        return False
    if rp is not None:
        raise ValueError(f"{what}: Takes(sv > 0) and repair= exclude each other (repair's keep rule scores without the speaker term)")
    if not eng.has("sv"):
        raise ValueError(f"{what}: Takes(sv > 0) needs the verifier part (SmallTTS(verifier=True) or get_engine(parts=(..., 'sv')))")
    if ns is not None and any(n < SV_MIN_FRAMES or n > ALIGN_MAX_FRAMES for n in ns):
        raise ValueError(f"{what}: Takes(sv > 0) needs {SV_MIN_FRAMES} to {ALIGN_MAX_FRAMES} frames in every row (a shorter row has no "
                         f"speaker embedding), got {min(ns)} .. {max(ns)}")
    if voices is not None and any(v.speaker is None for v in voices):
        raise ValueError(f"{what}: Takes(sv > 0) needs a Voice with a speaker embedding (encode it on an engine with the verifier part, "
                         f"from {SV_MIN_FRAMES} to {ALIGN_MAX_FRAMES} reference frames)")
    if voices is None and rs is not None and any(r < SV_MIN_FRAMES or r > ALIGN_MAX_FRAMES for r in rs):
        raise ValueError(f"{what}: Takes(sv > 0) needs {SV_MIN_FRAMES} to {ALIGN_MAX_FRAMES} reference frames in every row "
                         f"(a shorter reference has no speaker embedding)")
    return True


def _read_repair(recs: Sequence[_Batch]) -> List[tuple]:
    """What repair= left in finished batches, in ONE small read-back: per row of all records in order -> (kept (rounds,) int32,
    counts (rounds, 2) int32 = (bad tokens, freed frames) of every round's plan, before (rounds,) fp32 and after (rounds,) fp32, the
    row's total entering and leaving every round)."""
    parts = []
    for rec in recs:
        parts += [t.reshape(-1) for t in rec.rp_kept] + [t.reshape(-1) for t in rec.rp_counts] + [t.view(torch.int32) for t in rec.rp_totals]
    flat = torch.cat(parts).cpu().numpy()
    out, pos = [], 0
    for rec in recs:
        R, G = len(rec.rp_kept), int(rec.rp_kept[0].shape[0])
        kept = flat[pos: pos + R * G].reshape(R, G)
        counts = flat[pos + R * G: pos + 3 * R * G].reshape(R, G, 2)
        tot = flat[pos + 3 * R * G: pos + (4 * R + 1) * G].view(np.float32).reshape(R + 1, G)
        pos += (4 * R + 1) * G
        out += [(kept[:, g].copy(), counts[:, g].copy(), tot[:-1, g].copy(), tot[1:, g].copy()) for g in range(G)]
    return out


def _rows(audio: np.ndarray, ns: Sequence[int]) -> List[np.ndarray]:
    """A decoded batch on the host -> its rows (1, HOP_SIZE * n_b): the decoder is causal, so the prefixes are exact."""
    return [audio[b, :, : HOP_SIZE * n] for b, n in enumerate(ns)]


def _to_output_samples(dv: Optional["Delivery"], segs: List[tuple], words: Optional[List[tuple]]):
    """Segments (offset, n, start, gain) and words (index, kind, start, end) in 24 kHz samples -> the same in the Delivery's output
    samples, ceil(up * s / down) of every position, a length as the difference of its two ends.  dv None: as they are."""
    if dv is None:
        return segs, words
    segs = [(dv.samples(o), dv.samples(o + n) - dv.samples(o), dv.samples(st), g) for o, n, st, g in segs]
    words = None if words is None else [(i, kind, dv.samples(a), dv.samples(b)) for i, kind, a, b in words]
    return segs, words


RETIME_MAX_ROWS = 64                                   # rows of a long retiming that ride in one engine.retime call


def _retimed_words(words, table):
    """Word rows (align_words' six columns or synthesize_long's four) with start and end mapped through retime_times."""
    if words is None:
        return None
    k = lambda w: 3 if len(w) >= 6 else 2              # the column of the start
    return [tuple(w[:k(w)]) + (int(retime_times(int(w[k(w)]), table)), int(retime_times(int(w[k(w) + 1]), table))) + tuple(w[k(w) + 2:])
            for w in words]


def _retimed_segments(segs, table):
    """Segments (offset, n, start, gain) on the joined waveform -> on the retimed one: both ends through retime_times."""
    out = []
    for o, n, st, g in segs:
        a, b = int(retime_times(int(o), table)), int(retime_times(int(o) + int(n), table))
        out.append((a, b - a, st, g))
    return out


def _long_retime(what: str, retime, pcm16: bool) -> Optional["Retime"]:
    """The retime= argument of synthesize_long and render_long: a speed or a duration for the joined waveform."""
    rt = as_retime(retime)
    if rt is None:
        return None
    if rt.to_words is not None:
        raise ValueError(f"{what}: retime= takes a speed or a duration here; the words are not on the host before the join: align the "
                         "waveform and call SmallTTS.retime(audio, Retime(to_words=...), words=...)")
    if pcm16:
        raise ValueError(f"{what}: retime= and pcm16=True exclude each other: ask for deliver=Delivery(24000, 'pcm16')")
    return rt


def _piece_rows(off, seg, gain, spans, latents, winner, toks, ns, seeds, n_prefix: int, ep: Optional["Endpointing"],
                return_words: bool, return_pieces: bool, index0: int):
    """The pieces of one group of a long text from what was read back for its rows, host arrays only; row r speaks the piece of
    tokens toks[r] (the n_prefix prepended ones included), ns[r] frames and seed seeds[r].  off[r]: the row's offset in the joined
    waveform; with `ep` seg[r] = (start, n), its speech window, and gain[r]; with return_words (and for the Pieces' spans) spans[r]
    (P, 2); with return_pieces latents[r] (N, 64) and winner[r], the take that was kept (None: the piece's own seed).  index0: the
    words counted in front of this group.  -> (segments, words or None, Pieces or None), positions in 24 kHz samples."""
    segs, words, made = [], ([] if return_words else None), ([] if return_pieces else None)
    for r, (tok, n) in enumerate(zip(toks, ns)):
        segs.append((int(off[r]), HOP_SIZE * n, 0, 1.0) if ep is None else (int(off[r]), int(seg[r][1]), int(seg[r][0]), float(gain[r])))
        if return_words:
            words += word_times(token_groups(tok[n_prefix:]), spans[r], n, token0=n_prefix,
                                window=(segs[-1][2], segs[-1][1]) if ep is not None else None, offset=segs[-1][0],
                                index0=index0 + len(words))
        if return_pieces:
            made.append(Piece(tok, n_prefix, latents[r][:n], seeds[r] if winner is None else take_seed(seeds[r], int(winner[r])),
                              spans[r][: len(tok)] if return_words else None))
    return segs, words, made


class _Scoring(NamedTuple):
    """What the take scoring and the repair rounds of one synthesize_batch call read besides the device tensors: host values that
    no pass of the call changes, so that the first pass and the guard's rerun() enqueue the same work.  G caller rows, each spoken by
    the K sampler rows g * K .. g * K + K - 1."""
    K: int
    tk_run: "Takes"                      # the weights and thresholds of the total
    ctc_w: float                         # Takes.ctc where the CTC term is on, else 0
    sv_w: float                          # Takes.sv where the speaker term is on, else 0
    s_ns: List[int]                      # per sampler row: frames, prefix lengths, token counts
    s_p0s: List[int]
    s_ps: List[int]
    ns: List[int]                        # per caller row: frames, prefix lengths, token counts, reference frames
    p0s: List[int]
    ps: List[int]
    rs: List[int]
    ref: np.ndarray                      # (G * K, Rm, 64), (G * K, Pm): the sampler rows' references and tokens
    ids: np.ndarray
    voices: Optional[List["Voice"]]      # per caller row, or None (ref_latents)
    al_run: Optional["Alignment"]
    num_steps: int
    Nm: int
    rp: Optional["Repair"] = None
    rp_seeds: Optional[List[List[int]]] = None   # repair: per round, per caller row
    g_ref: Optional[np.ndarray] = None   # repair: the conditions' inputs, the frame mask and the caller's pins at G rows
    g_ids: Optional[np.ndarray] = None
    g_pm: Optional[np.ndarray] = None
    g_mask: Optional[np.ndarray] = None
    g_keep: Optional[np.ndarray] = None


def _score_takes(eng: HipEngine, c: _Scoring, x, mass, spans, score):
    """Scores every sampler row and keeps one per caller row, on the current stream: engine.take_scores, the CTC and speaker terms
    where they are on, engine.take_select with K > 1.  -> (x, mass, spans, winner, total, feat, nll, cos); x, mass and spans are the
    winners' with K > 1."""
    winner = nll = cos = None
    feat, total = eng.take_scores(mass, spans, score, c.s_ns, c.s_p0s, c.s_ps, c.tk_run)
    if c.ctc_w > 0.0:                                          # the CTC term: total' = total + (ctc * nll) / tokens, single fp32 operations
        tok = torch.from_numpy(c.ids.astype(np.int32)).pin_memory().to(eng.device, non_blocking=True)
        pw = torch.tensor([float(max(0, p1 - p0)) for p0, p1 in zip(c.s_p0s, c.s_ps)], dtype=torch.float32).pin_memory()
        nll = eng.ctc_score(eng.asr_logprobs(x, c.s_ns), [ASR_UPSAMPLE * n for n in c.s_ns], tok, c.s_p0s, c.s_ps)
        total = total + (nll * c.ctc_w) / pw.to(eng.device, non_blocking=True)
    if c.sv_w > 0.0:                                           # the speaker term: total' = total + sv * (1 - cos), single fp32 operations
        spk = (torch.stack([v.speaker for v in c.voices]) if c.voices is not None
               else eng.sv_embed(eng._dev(np.ascontiguousarray(c.ref[::c.K]), torch.float32), c.rs))
        cos = eng.sv_cosine(eng.sv_embed(x, c.s_ns), spk, c.K)
        total = total + (1.0 - cos) * c.sv_w
    if c.K > 1:
        x, _n, spans, mass, winner = eng.take_select(total, c.K, x, c.s_ns, spans, mass)
    return x, mass, spans, winner, total, feat, nll, cos


def _repair_rounds(eng: HipEngine, c: _Scoring, cache, x, mass, spans, winner, total, feat):
    """The repair rounds of the G caller rows, on the current stream: the winners' latents are the pins, x, spans and mass are merged
    in place.  -> (kept, counts per round, the rows' totals before round 1 and after every round)."""
    G = len(c.ns)
    if c.K > 1:                                                # the cache has G * K rows: the conditions again at G rows
        cache = eng.cond_encode(c.g_ref, np.asarray(c.rs, np.int64), c.g_ids, c.g_pm)
        if c.voices is not None:
            cache.update(eng.voice_expand(c.voices))
        sel = winner.long() + torch.arange(0, G * c.K, c.K, device=eng.device)
        t_cur, f_cur = total[sel], feat[sel]                   # the winners' totals and features
    else:
        t_cur, f_cur = total, feat
    keep_d = None if c.g_keep is None else torch.from_numpy(c.g_keep).pin_memory().to(eng.device, non_blocking=True)
    rp_kept, rp_counts, rp_totals = [], [], [t_cur]
    for r in range(c.rp.rounds):
        plan, counts = eng.repair_plan(mass, spans, c.ns, c.p0s, c.ps, c.rp, keep_d)
        nz_r = eng.randn_rows(c.rp_seeds[r], c.ns, c.num_steps, n_max=c.Nm)
        x_new, mass_new = eng.sample(cache, c.g_mask, num_steps=c.num_steps, noise=nz_r, seed=0, align=c.al_run, x_pin=x,
                                     pin=plan, start_step=0)
        spans_new, score_new = eng.align_path(mass_new, c.ns, c.p0s, c.ps)[:2]
        f_new, t_new = eng.take_scores(mass_new, spans_new, score_new, c.ns, c.p0s, c.ps, c.tk_run)
        # x, spans and mass are merged in place; every round's small outputs are tensors of their own (the report reads them)
        t_cur, f_cur, kept = eng.repair_keep(t_cur, t_new, counts, f_cur, f_new, x, x_new, spans, spans_new, mass, mass_new)
        rp_kept.append(kept); rp_counts.append(counts); rp_totals.append(t_cur)
    return rp_kept, rp_counts, rp_totals


def detect_watermark(engine: HipEngine, audio, key: int, *, max_offset: int = 0, threshold: float = 6.0) -> List[Tuple[float, int, bool]]:
    """Looks for Watermark(key)'s mark in 24 kHz audio (include/smalltts_hip.h smtts_watermark_detect): `audio` one array
    or a list of rows, float32 or int16 (PCM16: divided by 32767).  -> per row (z, offset, present): the best score over the
    hypotheses "the row's first sample is stream sample o", o = 0 .. max_offset (audio cropped from the front), the lowest such o,
    and z >= threshold.  Where the key's mark is absent z is about N(0, 1) per offset: the default threshold of 6 lets through
    roughly (max_offset + 1) * 1e-9 false alarms.  The offsets are searched 65 536 per device call; needs no weights."""
    rows = [audio] if isinstance(audio, np.ndarray) else list(audio)
    key, max_offset = int(key), int(max_offset)
    if not 0 <= key < 2 ** 64:
        raise ValueError(f"detect_watermark: key must be in [0, 2^64), got {key}")
    if not 0 <= max_offset <= 2 ** 40:
        raise ValueError(f"detect_watermark: max_offset must be in [0, 2^40], got {max_offset}")
    if not rows:
        return []
    flat = []
    for r in rows:
        r = np.asarray(r)
        if r.dtype == np.int16:
            r = r.astype(np.float32) / np.float32(32767.0)
        elif r.dtype != np.float32:
            raise TypeError(f"detect_watermark: float32 or int16 audio wanted, got {r.dtype}")
        flat.append(np.ascontiguousarray(r.reshape(-1)))
    res: List[Tuple[float, int, bool]] = []
    for g0 in range(0, len(flat), 1024):                       # smtts_watermark_detect takes at most 1024 rows
        grp = flat[g0: g0 + 1024]
        lens = [len(r) for r in grp]
        x = np.zeros((len(grp), max(max(lens), 1)), np.float32)
        for b, r in enumerate(grp):
            x[b, : len(r)] = r
        xd = torch.from_numpy(x).to(engine.device)
        best_z = np.full(len(grp), -np.inf, np.float32)
        best_o = np.zeros(len(grp), np.int64)
        for o_lo in range(0, max_offset + 1, 65536):
            _T, _den, off, z = engine.watermark_detect(xd, lens, key, o_lo=o_lo, n_off=min(65536, max_offset + 1 - o_lo))
            z, off = z.cpu().numpy(), off.cpu().numpy()
            better = z > best_z                                # strictly: the lowest offset wins a tie
            best_z, best_o = np.where(better, z, best_z), np.where(better, off, best_o)
        res += [(float(best_z[b]), int(best_o[b]), bool(best_z[b] >= threshold)) for b in range(len(grp))]
    return res


class SmallTTS:
    """DMD few-step synthesis: condition-encode -> n-step sampler -> codec decode, all on one MI355X."""

    def __init__(self, cond_encoder_path: str = "assets/dmd/condition_encoder.onnx",
                 denoiser_path: str = "assets/dmd/denoiser.onnx",
                 codec_decoder_path: str = "assets/codec/decoder.onnx",
                 providers: Optional[Iterable[str]] = None, *, weights: Optional[str] = None, device: int = 0,
                 precision: str = DEFAULT_PRECISION, num_steps: int = NUM_STEPS, seed: Optional[int] = None,
                 engine: Optional[HipEngine] = None, device_ids: Optional[Sequence[int]] = None, recogniser: bool = False,
                 verifier: bool = False) -> None:
        """Keyword-only additions to the reference signature (infer/onnx.py:53-59): `weights`, `device`, `precision`,
        `num_steps`, `seed`, and `device_ids` — the GPUs `synthesize_sharded` spreads a request list over from THIS process
        (one weight replica, engine and host thread per GPU; under torch.distributed the process group is used instead).
        `recogniser=True` adds the latent phoneme recogniser (engine part "asr") to this instance's engine: transcribe(),
        ctc_score(), Takes(ctc=) and the alignment calls (align_phonemes(), align_words(), align_wav(), realign()) need it.  `verifier=True` adds the latent speaker verifier (engine part "sv"):
        speaker_embedding(), speaker_similarity(), a Voice's `speaker` and Takes(sv=) need it."""
        if device_ids:
            device = int(device_ids[0])
        parts = ("dit", "decoder", "encoder") + (("asr",) if recogniser else ()) + (("sv",) if verifier else ())
        self.engine = engine or get_engine(weights, device, precision, parts=parts)
        if not (self.engine.has("dit") and self.engine.has("decoder")):
            raise RuntimeError("SmallTTS needs DiT and codec-decoder weights")
        if recogniser and not self.engine.has("asr"):
            raise RuntimeError("SmallTTS(recogniser=True): the engine holds no recogniser part (asr.* tensors)")
        if verifier and not self.engine.has("sv"):
            raise RuntimeError("SmallTTS(verifier=True): the engine holds no verifier part (sv.* tensors)")
        self.num_steps = int(num_steps)
        self._seed = seed
        self._rng = np.random.default_rng(seed) if seed is not None else None
        self._replicas: List["SmallTTS"] = [self]
        for d in list(device_ids or [])[1:]:
            # a repeated device id is its own replica (own engine + weights): the threads must not share an engine
            eng = (HipEngine(int(d), precision) if int(d) in [r.engine.device_index for r in self._replicas]
                   else get_engine(weights, int(d), precision, parts=("dit", "decoder", "encoder")))
            if not eng.has("dit"):
                _load_weights_into(eng, weights or DEFAULT_WEIGHTS, ("dit", "decoder", "encoder"))
            # replica seeds are derived from (seed, replica index): with one shared seed every shard would draw the same noise
            # for its k-th batch (correlated outputs across GPUs)
            rseed = None if seed is None else int(np.random.SeedSequence([int(seed), len(self._replicas)]).generate_state(1, np.uint64)[0] >> 1)
            self._replicas.append(SmallTTS(engine=eng, num_steps=num_steps, seed=rseed))

    def _next_seed(self) -> int:
        # the reference draws noise from numpy's global RNG (infer/onnx.py:104); seeding numpy (or seed=)
        # therefore makes runs reproducible here too, while the normals themselves come from the GPU
        if self._rng is not None:
            return int(self._rng.integers(0, 2 ** 63 - 1))
        return int(np.random.randint(0, 2 ** 31 - 1)) * 2654435761 % (2 ** 63)

    def detect_watermark(self, audio, key: int, *, max_offset: int = 0, threshold: float = 6.0) -> List[Tuple[float, int, bool]]:
        """detect_watermark on this instance's engine: one array or a list of rows, float32 or int16 at 24 kHz -> per row
        (z, offset, present).  `max_offset`: how many samples the audio may have lost at its front."""
        return detect_watermark(self.engine, audio, key, max_offset=max_offset, threshold=threshold)

    def encode_voice(self, ref_latents) -> Voice:
        """(R, 64) reference latents -> Voice: the style encoder and the 12 reference K / V projections run once, at B = 1, without
        a text half (cond_encode with P = 0).  Pass it to synthesize_batch(voices=...) / synthesize_long as often as needed."""
        ref = np.asarray(ref_latents, np.float32)
        if ref.ndim != 2 or ref.shape[1] != 64 or ref.shape[0] < 1:
            raise ValueError(f"encode_voice: reference latents must be (R, 64) with R >= 1, got {ref.shape}")
        cache = self.engine.cond_encode(ref[None], np.asarray([ref.shape[0]], np.int64), np.zeros((1, 0), np.int64),
                                        np.zeros((1, 0), bool))
        speaker = None
        if self.engine.has("sv") and SV_MIN_FRAMES <= ref.shape[0] <= ALIGN_MAX_FRAMES:   # (a reference outside has no embedding)
            speaker = self.engine.sv_embed(self.engine._dev(ref[None], torch.float32), [int(ref.shape[0])])[0]
        return Voice(self.engine, cache["k_ref"], cache["v_ref"], speaker)

    def encode_voice_wav(self, audio, sr: int, trim=None) -> Voice:
        """Mono samples at `sr` Hz -> Voice: device resampler to 24 kHz, codec encoder (through Encoder.encode_reference and its
        cache), then encode_voice.  `trim` (True or an Endpointing): the resampled clip is cut to the speech the endpoint kernels
        find in it, [start, start + n) with n rounded DOWN to whole codec hops but never below one hop (a window that would then
        pass the clip's end is moved back), so that room tone at the ends does not spend reference frames; a clip without speech
        raises ValueError.  No gain is applied to a reference."""
        y = self.engine.resample(np.asarray(audio, np.float32).reshape(-1), int(sr), SAMPLE_RATE)
        ep = as_endpointing(trim)
        if ep is not None:
            y = y.reshape(-1).contiguous()
            total = int(y.numel())
            if total < HOP_SIZE:
                raise ValueError("encode_voice_wav: the clip is shorter than one codec hop")
            seg = self.engine.endpoints(y.view(1, 1, -1), None, ep, lens=[total])[0].cpu()
            start, n = int(seg[0, 0]), int(seg[0, 1])
            if n == 0:
                raise ValueError("encode_voice_wav: no speech found in the clip (an all-silent clip is not a voice)")
            n = max(HOP_SIZE, n // HOP_SIZE * HOP_SIZE)
            start = min(start, total - n)
            y = y[start:start + n]
        lat = Encoder(engine=self.engine).encode_reference(y.reshape(1, 1, -1))
        return self.encode_voice(lat[0].numpy())

    def _asr_rows(self, what: str, latents, lengths):
        """_latent_rows for the recogniser's calls: the part, at most 64 rows of at most 225 frames."""
        if not self.engine.has("asr"):
            raise ValueError(f"{what}: needs the recogniser part (SmallTTS(recogniser=True))")
        x, ns = self._latent_rows(what, latents, lengths)
        B, N = int(x.shape[0]), int(x.shape[1])
        if not (1 <= B <= ASR_MAX_ROWS and 1 <= N <= ALIGN_MAX_FRAMES):
            raise ValueError(f"{what}: at most {ASR_MAX_ROWS} rows of at most {ALIGN_MAX_FRAMES} frames (got {B} x {N})")
        return x, ns

    def _sv_rows(self, what: str, latents, lengths):
        """_latent_rows for the verifier's calls: the part, at most 64 rows, every row of 6 to 225 frames."""
        if not self.engine.has("sv"):
            raise ValueError(f"{what}: needs the verifier part (SmallTTS(verifier=True))")
        x, ns = self._latent_rows(what, latents, lengths)
        if not 1 <= len(ns) <= SV_MAX_ROWS:
            raise ValueError(f"{what}: at most {SV_MAX_ROWS} rows, got {len(ns)}")
        if any(n < SV_MIN_FRAMES or n > ALIGN_MAX_FRAMES for n in ns):
            raise ValueError(f"{what}: every row needs {SV_MIN_FRAMES} to {ALIGN_MAX_FRAMES} frames (a shorter row has no speaker "
                             f"embedding), got {min(ns)} .. {max(ns)}")
        if int(x.shape[1]) > ALIGN_MAX_FRAMES:                  # padding behind the longest row
            x = x[:, :max(ns)].contiguous()
        return x, ns

    def _latent_rows(self, what: str, latents, lengths):
        """-> (x (B, N, 64) fp32 on the device, frames per row): `latents` a (B, N, 64) array / tensor with `lengths` (None: N for every
        row), or a sequence of (n_b, 64) arrays (their own lengths)."""
        eng = self.engine
        if isinstance(latents, (np.ndarray, torch.Tensor)) and latents.ndim == 3:
            ns = [int(latents.shape[1])] * int(latents.shape[0]) if lengths is None else [int(v) for v in lengths]
            x = eng._dev(latents, torch.float32)
        else:
            rows = [np.asarray(r, np.float32) for r in latents]
            if lengths is not None:
                raise ValueError(f"{what}: lengths= belongs to a (B, N, 64) array; a list of rows carries its own lengths")
            ns = [int(r.shape[0]) for r in rows]
            x = np.zeros((len(rows), max(ns + [1]), 64), np.float32)
            for b, r in enumerate(rows):
                if r.ndim != 2 or r.shape[1] != 64:
                    raise ValueError(f"{what}: row {b} must be (frames, 64), got {r.shape}")
                x[b, :ns[b]] = r
            x = eng._dev(x, torch.float32)
        B, N = int(x.shape[0]), int(x.shape[1])
        if x.shape[2] != 64 or len(ns) != B or any(n < 0 or n > N for n in ns):
            raise ValueError(f"{what}: latents (B, N, 64) and one length in [0, N] per row")
        return x, ns

    def speaker_embedding(self, latents, lengths=None) -> np.ndarray:
        """(B, 192) float32: the latent speaker verifier's embedding of every row of latents (engine.sv_embed), not
        normalised; every row is computed as if it were alone.  latents / lengths as transcribe().  Needs SmallTTS(verifier=True);
        ValueError for a row under 6 or over 225 frames.  What the embedding is worth is unvalidated: no trained verifier checkpoint
        has ever been loaded."""
        x, ns = self._sv_rows("speaker_embedding", latents, lengths)
        return self.engine.sv_embed(x, ns).cpu().numpy()

    def speaker_similarity(self, latents, reference, lengths=None) -> List[float]:
        """Per row the cosine of its speaker embedding with the reference's (engine.sv_embed, engine.sv_cosine), in
        [-1, 1], higher = closer.  `reference`: a Voice (its `speaker`), one (R, 64) array of reference latents for every row, or a
        sequence of such arrays, one per row.  ValueError for a row or a reference under 6 or over 225 frames, a Voice without an
        embedding, and without the verifier part.  Unvalidated on trained weights like speaker_embedding()."""
        what = "speaker_similarity"
        x, ns = self._sv_rows(what, latents, lengths)
        eng, B = self.engine, len(ns)
        if isinstance(reference, Voice):
            if reference.engine is not eng:
                raise ValueError(f"{what}: the Voice belongs to another engine")
            if reference.speaker is None:
                raise ValueError(f"{what}: the Voice has no speaker embedding (encode it on an engine with the verifier part, from "
                                 f"{SV_MIN_FRAMES} to {ALIGN_MAX_FRAMES} reference frames)")
            ref = reference.speaker[None].expand(B, -1).contiguous()
        else:
            one = isinstance(reference, (np.ndarray, torch.Tensor)) and reference.ndim == 2
            rx, rn = self._sv_rows(what + " (reference)", [reference] if one else list(reference), None)
            if not one and len(rn) != B:
                raise ValueError(f"{what}: one reference, or one per row ({B}), got {len(rn)}")
            ref = eng.sv_embed(rx, rn)
            if one:
                ref = ref.expand(B, -1).contiguous()
        return [float(v) for v in eng.sv_cosine(eng.sv_embed(x, ns), ref, 1).cpu().numpy()]

    def transcribe(self, latents, lengths=None) -> List[List[int]]:
        """Greedy phoneme ids of every row of latents: the recogniser's per-frame argmax (4 frames per latent frame), runs collapsed,
        blanks dropped (engine.asr_logprobs, engine.ctc_greedy).  latents: (B, N, 64) with `lengths` frames per row (None:
        all N), or a list of (n_b, 64) rows.  Needs SmallTTS(recogniser=True).  What the recogniser hears is unvalidated: no trained
        recogniser checkpoint has ever been loaded."""
        x, ns = self._asr_rows("transcribe", latents, lengths)
        eng = self.engine
        ids, n = eng.ctc_greedy(eng.asr_logprobs(x, ns), [ASR_UPSAMPLE * v for v in ns])
        flat = torch.cat([n, ids.reshape(-1)]).cpu().numpy()   # one read-back
        B = len(ns)
        T = int(ids.shape[1])
        return [flat[B + b * T: B + b * T + int(flat[b])].tolist() for b in range(B)]

    def ctc_score(self, latents, phoneme_ids: Sequence[Sequence[int]], lengths=None, prefix_lens=None) -> List[Tuple[float, float]]:
        """Per row (nll, nll / L): the CTC negative log-likelihood of the row's tokens phoneme_ids[b][prefix_lens[b]:] (L of them)
        under the recogniser's reading of its latents (engine.asr_logprobs, engine.ctc_score); +inf for a row without
        frames or tokens and for one with too few frames for its tokens.  latents / lengths as transcribe().  Lower = the phonemes
        were more probably spoken; what that is worth is unvalidated on trained weights."""
        x, ns = self._asr_rows("ctc_score", latents, lengths)
        toks, p0, tab = self._ctc_targets("ctc_score", len(ns), phoneme_ids, prefix_lens)
        eng = self.engine
        nll = eng.ctc_score(eng.asr_logprobs(x, ns), [ASR_UPSAMPLE * v for v in ns], eng._dev(tab, torch.int32), p0, [len(t) for t in toks])
        nll = nll.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            return [(float(v), float(np.float32(v) / np.float32(max(len(t) - p, 0)))) for v, t, p in zip(nll, toks, p0)]

    @staticmethod
    def _ctc_targets(what: str, B: int, phoneme_ids, prefix_lens):
        """The targets of a CTC call -> (token lists, prefix lengths, the zero-padded (B, P) int32 table)."""
        toks = [[int(t) for t in row] for row in phoneme_ids]
        p0 = [0] * B if prefix_lens is None else [int(v) for v in prefix_lens]
        if len(toks) != B or len(p0) != B or any(p < 0 or p > len(t) for p, t in zip(p0, toks)):
            raise ValueError(f"{what}: one token list and one prefix length in [0, tokens of the row] per row")
        P = max([len(t) for t in toks] + [1])
        if P > ALIGN_MAX_TOKENS:
            raise ValueError(f"{what}: at most {ALIGN_MAX_TOKENS} tokens per row, got {P}")
        tab = np.zeros((B, P), np.int32)
        for b, t in enumerate(toks):
            tab[b, :len(t)] = t
        return toks, p0, tab

    def align_phonemes(self, latents, phoneme_ids: Sequence[Sequence[int]], lengths=None, prefix_lens=None) -> List[tuple]:
        """Forced alignment: per row (spans, tok_logp, score) of the best CTC path of the row's tokens
        phoneme_ids[b][prefix_lens[b]:] through the recogniser's reading of its latents (engine.asr_logprobs, engine.ctc_align;
        DESIGN 8l).  spans (len(ids), 2) int32: the (first, last) RECOGNISER frame of every token, 4 per latent frame, 800 samples
        each; (-1, -1) for the prefix.  tok_logp (len(ids),) float32: the path's log-probability per token; score: its total.  A
        row that is not aligned (no frames, no tokens, fewer frames than its tokens and repeats need) has every span (-1, -1), tok_logp
        0 and score -inf.  latents / lengths as transcribe().  Works on any latents: a saved take, respeak's, an encoded recording.
        Needs SmallTTS(recogniser=True).  Only the mechanism is verified: no trained recogniser checkpoint has ever been loaded, so
        what these times are worth on speech is UNVALIDATED."""
        return self._align_rows("align_phonemes", latents, phoneme_ids, lengths, prefix_lens)[0]

    def _align_rows(self, what: str, latents, phoneme_ids, lengths, prefix_lens):
        x, ns = self._asr_rows(what, latents, lengths)
        toks, p0, tab = self._ctc_targets(what, len(ns), phoneme_ids, prefix_lens)
        eng = self.engine
        spans, tok_logp, score = eng.ctc_align(eng.asr_logprobs(x, ns), [ASR_UPSAMPLE * v for v in ns], eng._dev(tab, torch.int32), p0,
                                               [len(t) for t in toks])
        spans, tok_logp, score = spans.cpu().numpy(), tok_logp.cpu().numpy(), score.cpu().numpy()
        rows = [(spans[b, :len(t)].copy(), tok_logp[b, :len(t)].copy(), float(score[b])) for b, t in enumerate(toks)]
        return rows, toks, p0, ns

    def align_words(self, latents, phoneme_ids: Sequence[Sequence[int]], lengths=None, prefix_lens=None) -> List[List[tuple]]:
        """Word timings from align_phonemes: per row [(index, kind, phonemes, start sample, end sample, confidence), ...] for the
        token_groups of the row's own tokens (behind its prefix), by word_times at hop 800: samples at 24 kHz from the row's start,
        resolution 33.3 ms.  confidence: the mean over the group's tokens of tok_logp / span length (plans.group_confidence), the
        path's mean log-probability per frame, <= 0.  On a row that is not aligned every group collapses to (0, 0) with confidence
        -inf.  Arguments and limits as align_phonemes; UNVALIDATED on trained weights like it."""
        rows, toks, p0, ns = self._align_rows("align_words", latents, phoneme_ids, lengths, prefix_lens)
        out = []
        for (spans, tok_logp, _score), t, p, n in zip(rows, toks, p0, ns):
            groups = token_groups(t[p:])
            times = word_times(groups, spans, ASR_UPSAMPLE * n, token0=p, hop=CTC_HOP)
            conf = group_confidence(groups, spans, tok_logp, token0=p)
            out.append([(i, kind, g[1], s, e, c) for (i, kind, s, e), g, c in zip(times, groups, conf)])
        return out

    def align_wav(self, audio, sr: int, phoneme_ids: Sequence[int]) -> List[tuple]:
        """Word timings of a recording: mono samples at `sr` Hz, at most 30 s, and the phoneme ids of what it says -> align_words' row,
        times in samples at 24 kHz.  The clip goes through the device resampler and the codec encoder (Encoder.encode_reference and
        its cache, as encode_voice_wav), its latents through align_words.  Samples behind the last whole codec hop are not aligned."""
        a = np.asarray(audio, np.float32)
        if a.ndim != 1 and not (a.ndim == 2 and 1 in a.shape):
            raise ValueError(f"align_wav: a mono recording, got an array of shape {a.shape}")
        sr = int(sr)
        if sr < 1 or a.size < 1 or a.size > 30 * sr:
            raise ValueError(f"align_wav: between one sample and 30 s of audio at a positive rate, got {a.size} samples at {sr} Hz")
        if not self.engine.has("asr"):
            raise ValueError("align_wav: needs the recogniser part (SmallTTS(recogniser=True))")
        y = self.engine.resample(a.reshape(-1), sr, SAMPLE_RATE)
        if int(y.numel()) < HOP_SIZE:
            raise ValueError("align_wav: the clip is shorter than one codec hop")
        lat = Encoder(engine=self.engine).encode_reference(y.reshape(1, 1, -1))
        return self.align_words([lat[0].numpy()], [phoneme_ids])[0]

    # ---- long recordings: one row of any length up to 36 min ---------------------------------------------------------
    def _align_long(self, what: str, latents, phoneme_ids):
        """One recording through engine.asr_logprobs_long and engine.ctc_align_long -> ((spans, tok_logp, score), tokens, frames)."""
        eng = self.engine
        if not eng.has("asr"):
            raise ValueError(f"{what}: needs the recogniser part (SmallTTS(recogniser=True))")
        x = latents.detach() if isinstance(latents, torch.Tensor) else np.asarray(latents, np.float32)
        if x.ndim != 2 or int(x.shape[1]) != 64 or not 1 <= int(x.shape[0]) <= ASR_LONG_MAX_FRAMES:
            raise ValueError(f"{what}: one recording of (N, 64) latents, 1 <= N <= {ASR_LONG_MAX_FRAMES}, got {tuple(x.shape)}")
        toks = [int(t) for t in phoneme_ids]
        if len(toks) > CTC_LONG_MAX_TOKENS:
            raise ValueError(f"{what}: at most {CTC_LONG_MAX_TOKENS} tokens, got {len(toks)}")
        N = int(x.shape[0])
        tab = np.zeros((1, max(len(toks), 1)), np.int32)
        tab[0, :len(toks)] = toks
        logp = eng.asr_logprobs_long(eng._dev(x, torch.float32))
        spans, tok_logp, score = eng.ctc_align_long(logp[None], [ASR_UPSAMPLE * N], eng._dev(tab, torch.int32), [0], [len(toks)])
        spans, tok_logp, score = spans.cpu().numpy(), tok_logp.cpu().numpy(), score.cpu().numpy()
        return (spans[0, :len(toks)].copy(), tok_logp[0, :len(toks)].copy(), float(score[0])), toks, N

    def align_phonemes_long(self, latents, phoneme_ids: Sequence[int]) -> tuple:
        """align_phonemes for ONE recording past its limits: latents (N, 64), N <= 16384 (36 min), and at most 16383
        phoneme ids -> the (spans, tok_logp, score) of one row of align_phonemes.  The recogniser reads the recording in windows of
        30 s (engine.asr_logprobs_long), the path is found by engine.ctc_align_long; a recording inside align_phonemes' limits gives
        that call's bits.  A recogniser frame near a window cut has seen its 30 s window, not the whole recording.  UNVALIDATED on
        trained weights like align_phonemes."""
        return self._align_long("align_phonemes_long", latents, phoneme_ids)[0]

    def align_words_long(self, latents, phoneme_ids: Sequence[int], return_spans: bool = False):
        """align_words for ONE recording past its limits: [(index, kind, phonemes, start sample, end sample, confidence), ...], one
        row of align_words (token_groups, word_times at hop 800, group_confidence).  return_spans: (that list, spans (len(ids), 2)),
        e.g. for plans.speaking_rate.  Arguments and limits as align_phonemes_long."""
        (spans, tok_logp, _score), toks, N = self._align_long("align_words_long", latents, phoneme_ids)
        groups = token_groups(toks)
        times = word_times(groups, spans, ASR_UPSAMPLE * N, token0=0, hop=CTC_HOP)
        conf = group_confidence(groups, spans, tok_logp, token0=0)
        words = [(i, kind, g[1], s, e, c) for (i, kind, s, e), g, c in zip(times, groups, conf)]
        return (words, spans) if return_spans else words

    def encode_wav_long(self, y: torch.Tensor, enc_frames: int = 1024, enc_context: int = 32) -> torch.Tensor:
        """Latents (N, 64), on the device, of mono samples at 24 kHz (1-d, on the device), N = samples // hop.  At most enc_frames
        codec frames: one codec encode.  Longer: segments of enc_frames frames; every segment but the first is encoded together
        with the enc_context frames of audio in front of it, whose latents are dropped.  The encoder is causal, so context in
        front is all a segment can miss; how far the default 32 frames reach into its receptive field: DESIGN 8m."""
        eng = self.engine
        enc_frames, enc_context = int(enc_frames), int(enc_context)
        if enc_frames < 1 or enc_context < 0:
            raise ValueError(f"encode_wav_long: enc_frames >= 1 and enc_context >= 0, got {enc_frames}, {enc_context}")
        hop = eng.hop
        n = int(y.numel()) // hop
        if n <= enc_frames:
            return eng.codec_encode(y[:n * hop].reshape(1, 1, -1))[0]
        parts = []
        for f0 in range(0, n, enc_frames):
            f1, c = min(f0 + enc_frames, n), min(enc_context, f0)
            parts.append(eng.codec_encode(y[(f0 - c) * hop:f1 * hop].reshape(1, 1, -1))[0, c:])
        return torch.cat(parts)

    def align_wav_long(self, audio, sr: int, phoneme_ids: Sequence[int], enc_frames: int = 1024, enc_context: int = 32,
                       return_spans: bool = False):
        """align_wav for a recording of up to 36 min (16384 codec frames): mono samples at `sr` Hz and the phoneme ids of what it
        says (at most 16383) -> align_words_long's result, times in samples at 24 kHz.  The clip is resampled on the device,
        encoded by encode_wav_long (one encode up to enc_frames frames, else segments with enc_context frames of context; not
        through the reference cache) and aligned by align_words_long.  Samples behind the last whole codec hop are not aligned.
        On a clip inside align_wav's limits and enc_frames the result is align_wav's."""
        a = np.asarray(audio, np.float32)
        if a.ndim != 1 and not (a.ndim == 2 and 1 in a.shape):
            raise ValueError(f"align_wav_long: a mono recording, got an array of shape {a.shape}")
        sr = int(sr)
        if sr < 1 or a.size < 1:
            raise ValueError(f"align_wav_long: at least one sample at a positive rate, got {a.size} samples at {sr} Hz")
        if not self.engine.has("asr"):
            raise ValueError("align_wav_long: needs the recogniser part (SmallTTS(recogniser=True))")
        if a.size / sr * SAMPLE_RATE >= (ASR_LONG_MAX_FRAMES + 1) * HOP_SIZE:
            raise ValueError(f"align_wav_long: at most {ASR_LONG_MAX_FRAMES} codec frames ({ASR_LONG_MAX_FRAMES * HOP_SIZE / SAMPLE_RATE / 60:.1f} "
                             f"min) of audio, got {a.size / sr / 60:.1f} min")
        y = self.engine.resample(a.reshape(-1), sr, SAMPLE_RATE)
        n = int(y.numel()) // HOP_SIZE
        if n < 1:
            raise ValueError("align_wav_long: the clip is shorter than one codec hop")
        if n > ASR_LONG_MAX_FRAMES:
            y = y[:ASR_LONG_MAX_FRAMES * HOP_SIZE]
        return self.align_words_long(self.encode_wav_long(y, enc_frames, enc_context), phoneme_ids, return_spans=return_spans)

    def realign(self, pieces: Sequence[Piece]) -> List[Piece]:
        """The Pieces of a take with `spans` replaced by the recogniser's: align_phonemes on every piece's latents and tokens (its
        prefix left out), mapped to codec frames by plans.codec_spans, (first // 4, last // 4), (-1, -1) kept.  frames_of_groups,
        respeak and render_long then work from the CTC alignment instead of the text-attention tap's; tokens, latents and seeds are
        untouched, so the audio of the take does not change.  A piece that is not aligned keeps its old spans.  At most 64 pieces per
        call go through the recogniser at once; more are taken in turns."""
        pieces = list(pieces)
        if any(not isinstance(p, Piece) for p in pieces):
            raise ValueError("realign: a sequence of Pieces (synthesize_long(return_pieces=True), load_take)")
        if not self.engine.has("asr"):
            raise ValueError("realign: needs the recogniser part (SmallTTS(recogniser=True))")
        out = []
        for i in range(0, len(pieces), ASR_MAX_ROWS):
            grp = pieces[i: i + ASR_MAX_ROWS]
            rows = self.align_phonemes([p.latents for p in grp], [p.tokens for p in grp], prefix_lens=[p.prefix_len for p in grp])
            for p, (spans, _tok_logp, score) in zip(grp, rows):
                aligned = score > float("-inf")                # (False for NaN)
                out.append(Piece(p.tokens, p.prefix_len, p.latents, p.seed, codec_spans(spans) if aligned else p.spans))
        return out

    def synthesize_batch(self, ref_latents: Optional[Sequence[np.ndarray]], phoneme_ids: Sequence[Sequence[int]],
                         durations, *, noise: Optional[np.ndarray] = None, return_latents: bool = False,
                         frames: Optional[Sequence[int]] = None, _defer: bool = False,
                         voices: Optional[Sequence[Voice]] = None, seeds: Optional[Sequence[int]] = None, trim=None,
                         align=None, prefix_lens: Optional[Sequence[int]] = None, return_alignment: bool = False,
                         pins: Optional[Sequence[Optional[tuple]]] = None, start_step: int = 0, takes=None, return_takes: bool = False,
                         repair=None, return_repair: bool = False, _decode: bool = True, deliver=None,
                         watermark=None):
        """Batched synthesize: per-utterance (R_i,64) refs, token lists and durations -> list of (1, samples).
        `frames` overrides the per-utterance frame counts (default floor(duration * 7.5), infer/onnx.py:84; the HTTP server
        rounds up like the reference's Rust server, pipeline.rs:66).
        `voices`: B Voice objects (encode_voice) instead of `ref_latents` (pass None): only the text half of the condition encoder
        runs, the reference half is gathered from the voices.  `seeds`: B integers; row b's noise is the (seeds[b], step) Philox
        stream, so its latents do not depend on its batch-mates' seeds, lengths or order (not together with `noise`).
        `trim` (True or an Endpointing): row b comes back as (1, n_b), the window of its speech (engine.endpoints), times the
        row's gain when the Endpointing sets a level; cut and levelled on the device, so only the windows are copied out.
        `align` (True = Alignment(), or an Alignment; its default selection is unvalidated on trained weights): the sampler taps the
        DiT's text attention, the monotone path is found on the device (engine.align_path) and the call additionally returns, as
        the LAST element, per row [(group index, kind, start sample, end sample), ...] for the row's token_groups, in samples of
        the returned row (with `trim`: intersected with the speech window and counted from its start); resolution one codec
        frame (3200 samples).  `prefix_lens`: per row, how many leading tokens are a prepended transcription the audio does not
        speak; they are left out of the path and of the groups.  Rows of at most 225 frames and 198 tokens.
        `return_alignment`: one more element behind the words, per row (mass (n_b, P_b) fp32, spans (P_b, 2) int32).
        `pins`: one entry per row, None or (latents (n_b, 64) fp32, keep (n_b,) bool): the kept frames come back as given, bit for
        bit, and the sampler denoises the others with them in view (engine.sample x_pin / pin; smtts_sample_pinned).  The codec is
        causal, so the audio in front of the first free frame is that of the kept latents.  `start_step` = k > 0 runs only the
        sampler steps from k on, from the given latents (every row needs them then).  Works with every other argument; the fp16
        range guard's re-run uses the same pins.  Only the mechanism is verified: how well the 4-step student inpaints is
        UNVALIDATED on trained weights (every weight this project has run is seeded noise).
        `takes` (an int K or a Takes): every row is sampled K times and only the best-aligned take is decoded.  Row g
        becomes the K sampler rows g * K + k, which share its tokens, frames, voice or reference and pins and draw their noise from
        take_seed(seed_g, k), seed_g = seeds[g], or piece_seed(a fresh draw, g) without `seeds` (not together with `noise`).  On
        the batch's stream: the condition encoder and the sampler on G * K rows with the text-attention tap (`align` chooses the
        Alignment, default Alignment(); its limits of 225 frames and 198 tokens apply, and `prefix_lens` keeps a prepended
        transcription out of the path and the score also without `align`), engine.align_path, engine.take_scores,
        engine.take_select, then the codec and the endpoints on the G winners only, so that every other argument works as on a
        batch of G rows (words, return_alignment and return_latents are the winners').  At most 64 sampler rows (G * K).  K = 1 is
        the call without `takes`, bit for bit.  `return_takes`: one more element at the very end, per row (winner k, the winner's
        seed, totals (K,) fp32, features (K, 4) int32 = (cells, skipped, longest, idle)), from one small read-back (K = 1: the
        tap and the score run for it; without `seeds` the seed reported is the batch's).  What the score is worth is UNVALIDATED on
        trained weights (Takes).
        `repair` (an int = rounds, or a Repair): behind the sampler and the take selection, on the batch's stream and
        without a read-back, `rounds` times: engine.repair_plan pins every frame of the G rows but those of the badly aligned tokens
        (the caller's `pins` stay pinned whatever the plan says), one pinned sampler pass on G rows draws only the freed frames
        again, from repair_seed(seed_g, r) with the row's current latents in view, engine.align_path and engine.take_scores score
        the result, and engine.repair_keep replaces the row only where its total is strictly lower.  A frame the plan pinned keeps
        its bits; a row with nothing bad comes back as without `repair`, bit for bit.  Repair implies the tap, the path and the
        score as return_takes does (the total's weights are the Takes', Takes(1)'s without `takes`), and everything else works on
        the merged rows.  Not together with `noise` or `start_step` > 0.  `return_repair`: one more element at the very end, per
        row (kept (rounds,), (bad tokens, freed frames) (rounds, 2), total before (rounds,), total after (rounds,)), from one small
        read-back.  Only the mechanism is verified: whether the 4-step student inpaints audibly well, and whether a lower total
        is the better take, are UNVALIDATED on trained weights (Repair).
        `deliver` (a Delivery, a rate or a (rate, encoding) pair): behind the decode, on the batch's stream, every row is
        resampled to the Delivery's rate and encoded on the device (engine.deliver, one launch whatever B is) and only that is copied
        out: row b comes back as (1, rate * ns[b] / 7.5) samples in the encoding's dtype (float32, int16, or uint8 G.711 codes), and
        the words of `align` are given in output samples.  Not together with `trim`.  None is the call as it always was: 24 kHz
        fp32, not one launch more.
        `watermark` (a Watermark, a key or a (key, strength) pair): every row is marked on the device in front of the
        delivery (each row a stream of its own); without `deliver` it means Delivery(24000, "f32").  24 kHz, f32 or pcm16 only."""
        ep = as_endpointing(trim)
        al = as_alignment(align)
        tk = as_takes(takes)
        rp = as_repair(repair)
        wm, dv = marked_delivery("synthesize_batch", watermark, as_delivery(deliver))
        if dv is not None and ep is not None:
            raise ValueError("synthesize_batch: deliver= (and with it watermark=) and trim= exclude each other")
        if dv is not None and _defer:
            raise ValueError("synthesize_batch: a deferred batch is delivered by its caller (engine.deliver)")
        if tk is None and return_takes:
            raise ValueError("synthesize_batch: return_takes= belongs to takes=")
        if tk is not None and noise is not None:
            raise ValueError("synthesize_batch: noise= and takes= exclude each other")
        if rp is None and return_repair:
            raise ValueError("synthesize_batch: return_repair= belongs to repair=")
        if rp is not None and (noise is not None or int(start_step) > 0):
            raise ValueError("synthesize_batch: repair= excludes noise= and start_step > 0")
        K = 1 if tk is None else tk.k
        scored = (tk is not None and (K > 1 or return_takes)) or rp is not None   # the tap, the path and the score run for these
        tk_run = tk if tk is not None else Takes(1)            # the weights and thresholds of the total
        ctc_w = tk.ctc if check_takes_ctc("synthesize_batch", tk, rp, self.engine) and scored else 0.0
        if al is None and (return_alignment or (prefix_lens is not None and not scored)):   # (scored takes align too: they take prefix_lens)
            raise ValueError("synthesize_batch: prefix_lens= and return_alignment= belong to align=")
        sv_on = check_takes_sv("synthesize_batch", tk, rp, self.engine) and scored   # (rows and references: below, once they are known)
        if voices is not None:
            if ref_latents is not None:
                raise ValueError("synthesize_batch: pass either ref_latents or voices (with ref_latents=None), not both")
            if any(v.engine is not self.engine for v in voices):
                raise ValueError("synthesize_batch: a Voice belongs to another engine")
            ref_latents = [np.zeros((0, 64), np.float32)] * len(voices)   # the text half alone: cond_encode skips R = 0
        if seeds is not None and noise is not None:
            raise ValueError("synthesize_batch: noise= and seeds= exclude each other")
        B = len(ref_latents)
        if B == 0:
            return []
        if (voices is not None and len(phoneme_ids) != B) or (seeds is not None and len(seeds) != B):
            raise ValueError(f"synthesize_batch: {B} rows, {len(phoneme_ids)} token lists"
                             + (f", {len(seeds)} seeds" if seeds is not None else ""))
        if np.isscalar(durations):
            durations = [float(durations)] * B
        ns = [int(f) for f in frames] if frames is not None else [_frames(d) for d in durations]
        rs = [int(np.asarray(r).shape[0]) for r in ref_latents]
        ps = [len(p) for p in phoneme_ids]
        if sv_on:
            check_takes_sv("synthesize_batch", tk, rp, self.engine, ns, voices, rs)
        sv_w = tk.sv if sv_on else 0.0
        if tk is not None and B * K > Takes.MAX_ROWS:
            raise ValueError(f"synthesize_batch: takes= runs at most {Takes.MAX_ROWS} sampler rows, got {B} rows x {K} takes")
        al_run = al if (al is not None or not scored) else Alignment()
        rows = [g for g in range(B) for _k in range(K)]        # sampler row g * K + k speaks caller row g (K = 1: the rows themselves)
        Bs = len(rows)
        s_ns, s_rs, s_ps = [ns[g] for g in rows], [rs[g] for g in rows], [ps[g] for g in rows]
        Rm, Pm, Nm = (0 if voices is not None else max(max(rs), 1)), max(max(ps), 1), max(ns)
        ref = np.zeros((Bs, Rm, 64), np.float32)
        ids = np.zeros((Bs, Pm), np.int64)
        pm = np.zeros((Bs, Pm), bool)
        mask = np.zeros((Bs, Nm), bool)
        for b, g in enumerate(rows):
            ref[b, :rs[g]] = np.asarray(ref_latents[g], np.float32)
            ids[b, :ps[g]] = np.asarray(list(phoneme_ids[g]), np.int64)
            pm[b, :ps[g]] = True
            mask[b, :ns[g]] = True
        eng = self.engine
        pinned = _check_pins(pins, ns, start_step, self.num_steps)
        pin_kw = {}
        if pinned is not None:
            x_pin, keep = np.zeros((Bs, Nm, 64), np.float32), np.zeros((Bs, Nm), bool)
            for b, g in enumerate(rows):
                if pinned[g] is not None:
                    x_pin[b, :ns[g]], keep[b, :ns[g]] = pinned[g]
            pin_kw = {"x_pin": x_pin, "pin": keep, "start_step": int(start_step)}
        if K > 1:                                              # every take draws its own rows of noise
            fresh = None if seeds is not None else self._next_seed()
            row_seeds = [int(v) for v in seeds] if seeds is not None else [piece_seed(fresh, g) for g in range(B)]
            s_seeds, seed = [take_seed(row_seeds[g], k) for g in range(B) for k in range(K)], 0
        else:
            seed = self._next_seed() if seeds is None else 0
            s_seeds, row_seeds = seeds, ([seed] * B if seeds is None else [int(v) for v in seeds])
        rp_kw = {}
        if rp is not None:                                     # every round draws its own rows of noise for the G rows
            base = row_seeds if (seeds is not None or K > 1) else [piece_seed(seed, g) for g in range(B)]
            g_sel = slice(None, None, K)                       # sampler row g * K speaks caller row g
            g_ref, g_ids, g_pm, g_mask = (np.ascontiguousarray(a[g_sel]) for a in (ref, ids, pm, mask))
            rp_kw = {"rp": rp, "rp_seeds": [[repair_seed(base[g], r) for g in range(B)] for r in range(1, rp.rounds + 1)],
                     "g_ref": g_ref, "g_ids": g_ids, "g_pm": g_pm, "g_mask": g_mask,
                     "g_keep": None if pinned is None else np.ascontiguousarray(pin_kw["pin"][g_sel])}
        voices = None if voices is None else list(voices)      # run() keeps them alive while the batch is in flight
        s_voices = None if voices is None else [voices[g] for g in rows]
        p0s = [0] * B if prefix_lens is None else [int(v) for v in prefix_lens]
        if al_run is not None:
            if Nm > ALIGN_MAX_FRAMES or Pm > ALIGN_MAX_TOKENS:
                raise ValueError(f"synthesize_batch: align= covers rows of at most {ALIGN_MAX_FRAMES} frames and {ALIGN_MAX_TOKENS} tokens "
                                 f"(got {Nm} frames, {Pm} tokens)")
            if len(p0s) != B or any(p < 0 or p > ps[b] for b, p in enumerate(p0s)):
                raise ValueError("synthesize_batch: prefix_lens needs one length in [0, tokens of the row] per row")

        s_p0s = [p0s[g] for g in rows]
        c = _Scoring(K, tk_run, ctc_w, sv_w, s_ns, s_p0s, s_ps, ns, p0s, ps, rs, ref, ids, voices, al_run, self.num_steps, Nm, **rp_kw)

        def run() -> _Batch:
            cache = eng.cond_encode(ref, np.asarray(s_rs, np.int64), ids, pm)
            if voices is not None:
                cache.update(eng.voice_expand(s_voices))
            nz = noise if s_seeds is None else eng.randn_rows(s_seeds, s_ns, self.num_steps, n_max=Nm)
            mass = spans = seg = gain = winner = total = feat = nll = cos = None
            rp_kept = rp_counts = rp_totals = None
            if al_run is None:
                x = eng.sample(cache, mask, num_steps=self.num_steps, noise=nz, seed=seed, **pin_kw)
            else:
                # the tap and the path ride on this batch's stream behind its sampler; a re-run (fp16 range guard) recomputes them
                x, mass = eng.sample(cache, mask, num_steps=self.num_steps, noise=nz, seed=seed, align=al_run, **pin_kw)
                spans, score = eng.align_path(mass, s_ns, s_p0s, s_ps)[:2]
            if scored:                                         # takes: score every sampler row, keep one per caller row
                x, mass, spans, winner, total, feat, nll, cos = _score_takes(eng, c, x, mass, spans, score)
            if rp is not None:                                 # repair: G rows from here on, the winners' latents are the pins
                rp_kept, rp_counts, rp_totals = _repair_rounds(eng, c, cache, x, mass, spans, winner, total, feat)
            audio = eng.codec_decode(x) if _decode else None   # (B, 1, HOP * Nm); causal => prefixes are exact (None: synthesize_stream decodes)
            if ep is not None:                                 # behind the decode, on the same stream
                seg, gain, _e = eng.endpoints(audio, ns, ep)
            return _Batch(audio, x, mass, spans, seg, gain, ns, run, winner, total, feat, nll, cos, rp_kept, rp_counts, rp_totals)

        rec = run()
        if _defer:                                             # synthesize_batches / synthesize_long / the server: stay on the device / stream
            return rec
        return self._finish_batch(rec, ep, None if al is None else (phoneme_ids, p0s, ps), return_latents, return_alignment,
                                  (K, row_seeds) if return_takes else None, return_repair, dv, wm)

    def _finish_batch(self, rec: _Batch, ep: Optional["Endpointing"], tokens: Optional[tuple], return_latents: bool,
                      return_alignment: bool, takes: Optional[tuple] = None, return_repair: bool = False,
                      dv: Optional["Delivery"] = None, wm: Optional["Watermark"] = None):
        """synthesize_batch's tail: one batch from the device to what the call returns.  `tokens` = (token lists, prefix lengths, token
        counts) with align=, else None; `takes` = (K, the rows' seeds) with return_takes, else None.
        -> rows[, latents][, words[, raw alignment]][, takes][, repair]; the rows alone are returned bare."""
        eng = self.engine
        B = len(rec.ns)

        def read_head(rec):
            if dv is None:
                return (rec.audio if ep is None else rec.seg).cpu().numpy(), None
            out, counts = eng.deliver(rec.audio, [eng.hop * n for n in rec.ns], dv.rate, dv.encoding, mark=wm)   # behind the decode, same stream
            return out.cpu().numpy(), counts
        head, counts = read_head(rec)                          # synchronises: the saturation counters are final
        if eng.check_fp16_range("synthesize"):                 # an fp16 operand clipped: the site is split-bf16 now, run again
            rec = rec.rerun()
            head, counts = read_head(rec)
        if dv is not None:
            outs = [head[b: b + 1, : counts[b]] for b in range(B)]
        elif ep is None:
            outs = _rows(head, rec.ns)
        else:                                                  # cut and levelled on the device: only the windows are copied out
            offs, S = plan_packed(head[:, 1], 0.0)
            packed = torch.zeros(S, device=eng.device)
            eng.stitch_seg(rec.audio, rec.seg, rec.gain if ep.level_dbfs is not None else None, offs, None, packed)
            packed = packed.cpu().numpy()
            outs = [packed[None, offs[b]: offs[b] + int(head[b, 1])] for b in range(B)]
        res = [outs]
        if return_latents:
            xl = rec.latents.cpu().numpy()
            res.append([xl[b, : rec.ns[b]] for b in range(B)])
        if tokens is not None:
            phoneme_ids, p0s, ps = tokens
            spans_h = rec.spans.cpu().numpy()                  # B * P * 2 ints: the only read-back the timings need
            words = []
            for b in range(B):
                groups = token_groups(list(phoneme_ids[b])[p0s[b]:ps[b]])
                win = None if ep is None else (int(head[b, 0]), int(head[b, 1]))
                words.append(word_times(groups, spans_h[b], rec.ns[b], token0=p0s[b], window=win))
            res.append([_to_output_samples(dv, [], row)[1] for row in words])
            if return_alignment:
                mh = rec.mass.cpu().numpy()
                res.append([(mh[b, : rec.ns[b], : ps[b]], spans_h[b, : ps[b]]) for b in range(B)])
        if takes is not None:
            K, row_seeds = takes
            win, tot, ft = _read_takes([rec], K)
            extra = _takes_extra([rec], K, B)                  # Takes(ctc > 0): the K values of nll too; Takes(sv > 0): then the K cosines
            res.append([(int(win[b]), take_seed(row_seeds[b], int(win[b])) if K > 1 else int(row_seeds[b]), tot[b], ft[b]) + extra[b]
                        for b in range(B)])
        if return_repair:
            res.append(_read_repair([rec]))
        return outs if len(res) == 1 else tuple(res)

    def synthesize_batches(self, batches: Sequence[tuple], in_flight: int = 3, release_workspaces: bool = False) -> List[list]:
        """Several independent batches, `in_flight` of them overlapping on the GPU.

        batches: [(ref_latents, phoneme_ids, durations), ...] as for synthesize_batch.  Batch i runs whole on HIP stream
        i % in_flight with its own workspace, so one batch's latency-bound phases (condition encoders, DiT) fill the
        CUs another batch's kernels leave idle (bench.py: 16 ms per 8 x 10 s batch against 20 ms one at a time).
        The engine runs in throughput tuning meanwhile; results equal a loop of synthesize_batch under that tuning bit for bit."""
        if in_flight <= 1 or len(batches) <= 1:
            return [self.synthesize_batch(*b) for b in batches]
        eng, dev = self.engine, self.engine.device
        pending = self._run_in_flight([lambda b=b: self.synthesize_batch(*b, _defer=True) for b in batches], in_flight)
        outs = [_rows(rec.audio.cpu().numpy(), rec.ns) for rec in pending]
        if release_workspaces:
            torch.cuda.synchronize(dev)
            eng.release_workspaces()
        return outs

    @contextlib.contextmanager
    def _throughput(self):
        """Throughput tuning around what is enqueued inside: unsplit GEMMs, capped persistent codec grids, no engine side stream (it
        would serialise the text encoders of all batches in flight); the caller's mode is restored afterwards."""
        prev_tuning = self.engine.set_tuning("throughput")
        try:
            yield
        finally:
            self.engine.set_tuning(prev_tuning)

    @contextlib.contextmanager
    def _in_flight_slot(self, stream, i: int):
        """One batch in flight: what is enqueued inside goes onto `stream` with the workspace `batch{i}`; the default workspace is
        selected again afterwards."""
        try:
            with torch.cuda.stream(stream):
                self.engine.use_workspace(f"batch{i}")
                yield
        finally:
            self.engine.use_workspace(None)

    def _run_in_flight(self, calls: Sequence[Callable[[], _Batch]], in_flight: int) -> List[_Batch]:
        """The machinery of synthesize_batches: calls[i]() enqueues one deferred batch and returns its record; call i runs whole on
        HIP stream i % in_flight with its own workspace under throughput tuning.  Returns the finished records, on the device, after
        the fp16 range guard has been honoured.  The guard's re-run happens after the caller's tuning and workspace have been
        restored: every batch again, one at a time, on the current stream — under the CALLER's tuning, not under throughput."""
        eng = self.engine
        dev = eng.device
        cur = torch.cuda.current_stream(dev)
        streams = [torch.cuda.Stream(dev) for _ in range(max(1, min(in_flight, len(calls))))]
        for st in streams:
            st.wait_stream(cur)
        pending = []
        with self._throughput():                               # held across the whole loop: the engine sees one change and one restore
            for i, call in enumerate(calls):
                with self._in_flight_slot(streams[i % len(streams)], i % len(streams)):
                    pending.append(call())
        for st in streams:
            cur.wait_stream(st)
        torch.cuda.synchronize(dev)
        if eng.check_fp16_range("synthesize_batches"):         # clipped somewhere: every batch again, one at a time, at the demoted precision
            pending = [rec.rerun() for rec in pending]
        return pending

    def _long_inputs(self, what: str, voice: Voice, text, token_lists, durations, prefix_tokens):
        """What synthesize_long and synthesize_long_stream speak: -> (prefix tokens, every piece's tokens with the prefix in front,
        frames per piece), from `text` (split_text, phonemised, estimate_duration) or from pre-split `token_lists` with `durations`."""
        if voice.engine is not self.engine:
            raise ValueError(f"{what}: the Voice belongs to another engine")
        prefix = [int(t) for t in (prefix_tokens or [])]
        if (text is None) == (token_lists is None):
            raise ValueError(f"{what}: pass either text or token_lists (with durations)")
        if text is not None:
            from .phonemes import get_token_ids
            pieces = split_text(text, max_tokens=198 - len(prefix))
            token_lists = [get_token_ids(p) for p in pieces]
            durations = [estimate_duration(p) for p in pieces]
        else:
            if durations is None or (not np.isscalar(durations) and len(durations) != len(token_lists)):
                raise ValueError(f"{what}: token_lists needs one duration per piece")
            if np.isscalar(durations):
                durations = [float(durations)] * len(token_lists)
        toks = [prefix + [int(t) for t in p] for p in token_lists]
        return prefix, toks, [_frames(d) for d in durations]

    def _long_request(self, what: str, voice: Voice, text, token_lists, durations, prefix_tokens, max_batch: int, pcm16: bool, trim,
                      align, return_words: bool, takes, repair, deliver, watermark,
                      reports: Optional[Tuple[bool, bool]] = None) -> "_LongRequest":
        """The argument front synthesize_long and synthesize_long_stream share, errors in one order for both: the options as their
        records, one take dropped, the align= rule, the pieces (_long_inputs), the speaker term's limits and the group size takes=
        allow.  `reports` = synthesize_long's (return_takes, return_repair), which also checks the CTC term here; None: the stream,
        which has no reports and whose batches check that term."""
        return_takes, return_repair = reports or (False, False)
        wm, dv = marked_delivery(what, watermark, as_delivery(deliver))   # (one mark stream for the text)
        if dv is not None and pcm16:
            raise ValueError(f"{what}: deliver= (and with it watermark=) and pcm16=True exclude each other: ask for "
                             "Delivery(rate, 'pcm16')")
        ep = as_endpointing(trim)
        tk = as_takes(takes)
        rp = as_repair(repair)
        if tk is None and return_takes:
            raise ValueError(f"{what}: return_takes= belongs to takes=")
        if rp is None and return_repair:
            raise ValueError(f"{what}: return_repair= belongs to repair=")
        if tk is not None and tk.k == 1 and not return_takes:
            tk = None                                          # one take and nothing to report: the call without takes
        if reports is not None:
            check_takes_ctc(what, tk, rp, self.engine)
        al = as_alignment(align if align is not None else (True if return_words else None))
        if al is not None and not return_words and tk is None and rp is None:
            raise ValueError(f"{what}: align= belongs to return_words=True")
        prefix, toks, ns = self._long_inputs(what, voice, text, token_lists, durations, prefix_tokens)
        check_takes_sv(what, tk, rp, self.engine, ns or None, [voice])   # every piece, in front of the first batch
        K = 1 if tk is None else tk.k
        if tk is not None and K * max_batch > Takes.MAX_ROWS:
            max_batch = Takes.MAX_ROWS // K                    # the sampler batch is K times the group
        return _LongRequest(wm, dv, ep, al, tk, rp, K, prefix, toks, ns, max_batch)

    def _long_calls(self, voice: Voice, toks, ns, seeds, groups, n_prefix: int, ep, al, tk, rp, return_takes: bool):
        """One deferred synthesize_batch per group of a long text, as synthesize_long and synthesize_long_stream enqueue them:
        -> (calls, the Alignment the batches run with or None)."""
        al_b = al if (al is not None or (tk is None and rp is None)) else Alignment()   # takes, repair: the path leaves the prefix out, as the words do
        # (return_takes with one take: the deferred batch returns its record either way, the flag makes it score its rows)
        kw = ({} if al_b is None else {"align": al_b}) if tk is None else {"align": al_b, "takes": tk, "return_takes": return_takes}
        if rp is not None:
            kw["repair"] = rp
        # with trim every batch enqueues its endpoints behind its decode, on its own stream: they overlap the other batches in flight
        calls = [lambda g=g: self.synthesize_batch(None, [toks[i] for i in g], None, frames=[ns[i] for i in g], voices=[voice] * len(g),
                                                   seeds=[seeds[i] for i in g], trim=ep, _defer=True,
                                                   **kw, **({} if al_b is None else {"prefix_lens": [n_prefix] * len(g)}))
                 for g in groups]
        return calls, al_b

    def synthesize_long(self, voice: Voice, text: Optional[str] = None, *, token_lists: Optional[Sequence[Sequence[int]]] = None,
                        durations: Optional[Sequence[float]] = None, seed: Optional[int] = None, gap_ms: float = 120.0,
                        fade_ms: float = 5.0, max_batch: int = 8, in_flight: int = 3, pcm16: bool = False,
                        prefix_tokens: Optional[Sequence[int]] = None, trim=None, return_segments: bool = False,
                        return_words: bool = False, align=None, return_pieces: bool = False, takes=None, return_takes: bool = False,
                        repair=None, return_repair: bool = False, deliver=None, watermark=None, retime=None):
        """A whole text in one voice -> one waveform (1, S), fp32 or (pcm16=True) int16 PCM, S = sum(3200 * n_i) + (pieces - 1) *
        round(gap_ms * 24).

        Either `text` (cut by split_text, phonemised, durations from estimate_duration per piece) or pre-split `token_lists` with
        `durations`.  Consecutive pieces ride in batches of at most `max_batch`, `in_flight` batches overlapping on the GPU under
        throughput tuning (the synthesize_batches machinery; always, also for a single batch, so that the result does not depend
        on how the text was grouped beyond the engine's batch-shape tolerance).  Only the text half of the condition encoder runs
        per batch; the voice was encoded once.  Piece i draws its noise from seed SeedSequence([seed, i]) -> 63 bits.  The rows are
        joined on the device (engine.stitch: `gap_ms` of silence between pieces, a raised-cosine fade of `fade_ms` at both ends of
        each, fade_table) and copied to the host once.  `prefix_tokens` (the reference clip's transcription) is prepended to every
        piece's tokens, as forward() prepends the transcription; the splitter's token budget shrinks by its length.

        `trim` (True = Endpointing(), or an Endpointing): a piece is as long as its guessed duration, whatever part of that is
        speech, so the pause at a join is `gap_ms` plus the dead air the guess left.  With `trim` the ends of the speech of every
        piece are found on the device (engine.endpoints, enqueued on each batch's own stream behind its decode), the table is read
        back once, and the join puts the speech windows `gap_ms` apart (plan_packed; a piece without speech takes no room), each
        times its gain when the Endpointing sets a level, faded over the window's own ends (engine.stitch_seg); S follows from the
        windows.  `return_segments=True`: -> (waveform, [(offset in the waveform, n, start inside the piece, gain), ...] per piece),
        the caller's subtitle / highlight timings (without trim: (offset, 3200 * n_i, 0, 1.0)).

        `return_words=True` (with `align`, an Alignment, to choose the tapped layers / heads / steps; the default selection is
        unvalidated on trained weights): additionally -> [(group index, kind, start sample, end sample), ...], the token_groups of
        every piece's own tokens (the prefix is left out) in text order, the index running through the whole text, on the joined
        waveform's timeline: a piece's words lie inside its segment (with trim: inside its speech window).  The tap and the path
        kernel are enqueued on each batch's own stream behind its sampler; the spans are read back once, 8 bytes per token.
        Resolution: one codec frame, 3200 samples.

        `return_pieces=True`: additionally -> [Piece(tokens, prefix_len, latents, seed), ...], what each piece was spoken from and
        its latents (one read-back from the finished batches): render_long(pieces, ...) with the same join parameters reproduces the
        waveform, and respeak makes the latents of a replacement piece.

        `takes` (an int K or a Takes; DESIGN 8d, what the score is worth is UNVALIDATED on trained weights): every piece is sampled K
        times, from take_seed(piece seed, k), and only the best-aligned take of each is decoded and joined
        (synthesize_batch(takes=)); `align` then chooses the tapped layers / heads / steps also without return_words.  The groups
        stay plan_long's, `max_batch` pieces per batch, so the decode batches have render_long's shapes while the sampler batch is K
        times larger; where K * max_batch would pass 64 sampler rows the group size is lowered to 64 // K, and render_long then
        reproduces the waveform when it is given that max_batch.  A Piece's `seed` is the winning take's seed.  K = 1 is the call
        without `takes`.  `return_takes=True`: additionally -> per piece (winner k, the winner's seed, totals (K,), features (K, 4)),
        from one small read-back.

        `repair` (an int = rounds, or a Repair; DESIGN 8e, UNVALIDATED on trained weights like `takes`): every group repairs its
        rows behind its sampler and take selection (synthesize_batch(repair=)), from repair_seed(piece seed, r); `align` then
        chooses the tapped layers / heads / steps also without return_words.  A Piece's latents are the repaired latents, so
        render_long reproduces the waveform as ever, while its `seed` stays what the piece was first spoken from: the repaired
        frames are not a function of that seed alone.  `return_repair=True`: additionally, as the very last element -> per piece
        (kept (rounds,), (bad tokens, freed frames) (rounds, 2), total before (rounds,), total after (rounds,)), from one small
        read-back.

        `deliver` (a Delivery, a rate or a (rate, encoding) pair): the JOINED waveform, one row, is resampled and encoded
        on the device behind the join (engine.deliver) and comes back as (1, ceil(up * S / down)) in the encoding's dtype; segment
        offsets, lengths and starts and the word times are then given in output samples, ceil(up * s / down) of the 24 kHz position
        (a length as the difference of its two ends).  The pieces' batches are not resampled one by one.  Not together with
        pcm16=True (ask for Delivery(rate, "pcm16")).  None is the call as it always was.
        `watermark` (a Watermark, a key or a (key, strength) pair): the JOINED waveform is marked on the device in front of
        the delivery, as one stream from sample 0; without `deliver` it means Delivery(24000, "f32").  24 kHz, f32 or pcm16 only.
        `retime` (a Retime with a speed or a duration, or a number = a speed): the JOINED waveform is retimed on the device
        (engine.retime: WSOLA, the pitch is kept) behind the join and in front of the watermark and the delivery, so that a mark is
        embedded in the samples that leave.  Retime(duration=d) gives exactly round(d * 24000) samples at 24 kHz.  Segments and words
        are mapped through plans.retime_times (a segment's start inside its piece stays a position in the piece).  Not with
        pcm16=True; Retime(to_words=...) belongs to SmallTTS.retime.  None is the call as it always was, Retime(speed=1.0) its bits.
        Returns (waveform[, segments][, words][, pieces][, takes][, repair])."""
        rt = _long_retime("synthesize_long", retime, pcm16)
        q = self._long_request("synthesize_long", voice, text, token_lists, durations, prefix_tokens, max_batch, pcm16, trim, align,
                               return_words, takes, repair, deliver, watermark, reports=(return_takes, return_repair))
        dv, ep, tk, K, toks, ns = q.dv, q.ep, q.tk, q.K, q.toks, q.ns
        groups, offsets, S = plan_long(ns, q.max_batch, gap_ms)

        def result(out, segs, words, made, taken=None, mended=None, table=None):   # words None: not aligned
            if table is not None:
                segs, words = _retimed_segments(segs, table), _retimed_words(words, table)
            segs, words = _to_output_samples(dv, segs, words)
            res = ((out,) + ((segs,) if return_segments else ()) + ((words,) if words is not None else ())
                   + ((made,) if return_pieces else ()) + ((taken,) if return_takes else ()) + ((mended,) if return_repair else ()))
            return res if len(res) > 1 else out

        if not toks:
            return result(np.zeros((1, 0), dv.dtype if dv is not None else np.int16 if pcm16 else np.float32), [],
                          [] if return_words else None, [], [], [])
        base = self._next_seed() if seed is None else int(seed)
        seeds = [piece_seed(base, i) for i in range(len(toks))]
        calls, _al_b = self._long_calls(voice, toks, ns, seeds, groups, len(q.prefix), ep, q.al, tk, q.rp, return_takes)
        out, segs, pending, table = self._join_long(calls, groups, ns, offsets, S, ep, in_flight, gap_ms, fade_ms, pcm16, dv, q.wm, rt)
        win = taken = None
        mended = _read_repair(pending) if return_repair else None   # one small read-back for the whole text
        if tk is not None and (return_takes or return_pieces):
            win, tot, ft = _read_takes(pending, K)             # one small read-back for the whole text
            extra = _takes_extra(pending, K, len(toks))        # Takes(ctc > 0): nll (K,) too; Takes(sv > 0): then cos (K,)
            # (what each piece was spoken from: the winner's seed)
            taken = [(int(win[i]), take_seed(seeds[i], int(win[i])), tot[i], ft[i]) + extra[i] for i in range(len(toks))]

        def read_rows(tensors, width):                         # one read-back for the whole text: every batch's table, flattened
            flat, pos, out = torch.cat([t.reshape(-1) for t in tensors]).cpu().numpy(), 0, []
            for g, t in zip(groups, tensors):
                out.append(flat[pos: pos + len(g) * int(t.shape[1]) * width].reshape(len(g), int(t.shape[1]), width))
                pos += out[-1].size
            return out
        spans = read_rows([rec.spans for rec in pending], 2) if return_words else [None] * len(groups)
        lats = read_rows([rec.latents for rec in pending], 64) if return_pieces else [None] * len(groups)
        words, made = ([] if return_words else None), ([] if return_pieces else None)
        for g, sp, xg in zip(groups, spans, lats):
            _segs, w, m = _piece_rows([segs[i][0] for i in g], [(segs[i][2], segs[i][1]) for i in g], [segs[i][3] for i in g], sp, xg,
                                      None if win is None else [win[i] for i in g], [toks[i] for i in g], [ns[i] for i in g],
                                      [seeds[i] for i in g], len(q.prefix), ep, return_words, return_pieces, len(words or ()))
            words, made = (words + w if return_words else None), (made + m if return_pieces else None)
        return result(out, segs, words, made, taken, mended, table)

    def _join_long(self, calls, groups, ns, offsets, S, ep: Optional["Endpointing"], in_flight: int, gap_ms: float, fade_ms: float,
                   pcm16: bool, dv: Optional["Delivery"] = None, wm: Optional["Watermark"] = None, rt: Optional["Retime"] = None):
        """The tail synthesize_long and render_long share: the deferred batches `calls` (one per group) run through _run_in_flight,
        their rows are joined on the device and copied out once.  With `ep` the records carry their endpoints (every batch enqueued
        them behind its decode, and so does its re-run): the tables are read back once and the join puts the speech windows `gap_ms`
        apart, which replaces `offsets` and `S`.  With `rt` the joined row is retimed behind the join, in front of the mark and the
        delivery.  -> (waveform (1, S), segments on the JOINED waveform, the finished batches, the retiming's anchor table or
        None: what maps the segments onto the waveform returned)."""
        eng = self.engine
        pending = self._run_in_flight(calls, in_flight)
        if ep is not None:
            seg_h = torch.cat([rec.seg for rec in pending]).cpu().numpy()     # one small read-back: 16 bytes per piece ...
            gain_h = torch.cat([rec.gain for rec in pending]).cpu().numpy()   # ... and 4
            offsets, S = plan_packed(seg_h[:, 1], gap_ms)
            segs = [(int(offsets[i]), int(seg_h[i, 1]), int(seg_h[i, 0]), float(gain_h[i])) for i in range(len(ns))]
        else:
            segs = [(offsets[i], HOP_SIZE * ns[i], 0, 1.0) for i in range(len(ns))]
        out = torch.zeros(S, dtype=torch.int16 if pcm16 else torch.float32, device=eng.device)
        w = fade_table(fade_ms)
        fade = torch.from_numpy(w).to(eng.device) if w.size else None
        for g, rec in zip(groups, pending):
            offs = [offsets[i] for i in g]
            if ep is None:
                eng.stitch(rec.audio, rec.ns, offs, fade, out)
            else:
                eng.stitch_seg(rec.audio, rec.seg, rec.gain if ep.level_dbfs is not None else None, offs, fade, out)
        table = None
        if rt is not None and S > 0:
            anchors, _clamped = retime_anchors(S, speed=rt.speed, duration=rt.duration)
            out, table = self._retime_device(out, anchors, None, rt)
            S = int(out.numel())
        if dv is not None:                                     # the joined waveform, one row, at the caller's rate and encoding
            if S == 0:
                return np.zeros((1, 0), dv.dtype), segs, pending, table
            d, cnt = eng.deliver(out.view(1, 1, S), [S], dv.rate, dv.encoding, mark=wm)
            return d[:, :cnt[0]].cpu().numpy(), segs, pending, table
        return out.cpu().numpy()[None], segs, pending, table

    # ---- retiming: WSOLA on the device onto a speed, a length or word times --------------------------------------------
    def _retime_device(self, y: torch.Tensor, anchors, words, rt: "Retime", max_row: int = 30 * SAMPLE_RATE):
        """y: 24 kHz samples, 1-d fp32 on the device, and the anchor table of their retiming -> (the retimed samples, 1-d on the
        device, the table in force).  Up to max_row samples in and out: one row, the table as given.  Longer: plans.retime_rows cuts
        rows (in aligned pauses of `words` where there are any), RETIME_MAX_ROWS of them ride in one engine.retime call, and
        engine.stitch_seg places them one behind the other (no fade, no gain); the table then holds the cuts.  Gathering a group is
        a host-side loop: one zeroed (rows, 1, longest row) tensor and one device-to-device slice copy per row, up to 64 per group;
        fine for rows of 30 s in a stage that is off by default, not built for throughput."""
        eng = self.engine
        rows, table = retime_rows(int(y.numel()), anchors, words, max_row=max_row)
        if len(rows) == 1:
            out, lens = eng.retime(y.view(1, 1, -1), [int(y.numel())], [rows[0][3]], hop=rt.hop, delta=rt.delta)
            return out.view(-1)[:lens[0]], table
        joined = torch.zeros(int(table[-1, 1]), device=eng.device)
        for g0 in range(0, len(rows), RETIME_MAX_ROWS):
            grp = rows[g0: g0 + RETIME_MAX_ROWS]
            batch = torch.zeros(len(grp), 1, max(r[1] for r in grp), device=eng.device)
            for b, (s0, sn, _d0, _tab) in enumerate(grp):
                batch[b, 0, :sn] = y[s0: s0 + sn]
            out, lens = eng.retime(batch, [r[1] for r in grp], [r[3] for r in grp], hop=rt.hop, delta=rt.delta)
            seg = eng._upload_i64([[0, n] for n in lens])
            eng.stitch_seg(out, seg, None, [r[2] for r in grp], None, joined)
        return joined, table

    def retime(self, audio, retime, *, words=None):
        """Retimes 24 kHz mono audio of any length on the device (engine.retime: WSOLA, the pitch is kept) -> (waveform
        (1, S_out) fp32, `words` mapped through plans.retime_times or None, the group indices of the words that were clamped).
        `retime`: a Retime, or a number = a speed.  Retime(speed=) / Retime(duration=): S_out = round(n / speed) / round(duration *
        24000).  Retime(to_words=rows): `words` says where the words are now (align_wav's or align_words' rows) and `rows` where they
        shall lie (plans.retime_anchors); every word that is not reported as clamped then starts and ends exactly at its target
        (reported is also a word that abuts the word in front or starts at sample 0 and was sent somewhere else).  Audio longer
        than 30 s is cut into rows in the middle of aligned pauses of `words` (plans.retime_rows).  How retimed speech sounds is
        untested: nobody has listened to it."""
        rt = as_retime(retime)
        if rt is None:
            raise ValueError("retime: a Retime (or a speed) is needed")
        a = audio.detach().cpu().numpy() if isinstance(audio, torch.Tensor) else np.asarray(audio)
        a = a.astype(np.float32, copy=False)
        if (a.ndim != 1 and not (a.ndim == 2 and 1 in a.shape)) or a.size < 1:
            raise ValueError(f"retime: mono audio of at least one sample, got an array of shape {a.shape}")
        if rt.to_words is not None and words is None:
            raise ValueError("retime: Retime(to_words=...) needs words=, where the words are now")
        n = int(a.size)
        anchors, clamped = retime_anchors(n, speed=rt.speed, duration=rt.duration, words=words if rt.to_words is not None else None,
                                          to_words=rt.to_words, min_rate=rt.min_rate, max_rate=rt.max_rate)
        y = torch.from_numpy(np.ascontiguousarray(a.reshape(-1))).to(self.engine.device)
        out, table = self._retime_device(y, anchors, words, rt)
        return out.cpu().numpy()[None], _retimed_words(None if words is None else list(words), table), clamped

    def retime_wav(self, audio, sr: int, phoneme_ids: Sequence[int], retime, long: bool = False):
        """A recording and what it says, retimed: mono samples at `sr` Hz are resampled to 24 kHz on the device, aligned (align_wav,
        or with long=True align_wav_long, for up to 36 min) and retimed -> retime()'s triple, the words being the alignment's rows
        mapped onto the result.  Needs SmallTTS(recogniser=True), like the aligners."""
        if not self.engine.has("asr"):
            raise ValueError("retime_wav: needs the recogniser part (SmallTTS(recogniser=True))")
        words = self.align_wav_long(audio, sr, phoneme_ids) if long else self.align_wav(audio, sr, phoneme_ids)
        y = self.engine.resample(np.asarray(audio, np.float32).reshape(-1), int(sr), SAMPLE_RATE)
        return self.retime(y.reshape(-1), retime, words=words)

    # ---- pitch: an F0 track on the device, f0 per word ---------------------------------------------------------------------
    def pitch(self, audio, pitch=None, words=None):
        """pitch_track on this instance's engine: the F0 track of 24 kHz mono audio of any length -> PitchTrack(f0, strength, hop, sr),
        with `words` (align_words' or align_wav's rows) -> (the track, [(row, dict(f0_median, f0_min, f0_max, voiced)), ...]).
        Checked on synthetic signals only: nothing is claimed about accuracy on speech."""
        return pitch_track(self.engine, audio, pitch, words)

    def pitch_wav(self, audio, sr: int, pitch=None, words=None):
        """pitch() of a recording at `sr` Hz (pitch_track_wav): resampled to 24 kHz on the device first, as align_wav does.  It does
        not need the recogniser."""
        return pitch_track_wav(self.engine, audio, sr, pitch, words)

    def synthesize_long_stream(self, voice: Voice, text: Optional[str] = None, *, token_lists: Optional[Sequence[Sequence[int]]] = None,
                               durations: Optional[Sequence[float]] = None, seed: Optional[int] = None, gap_ms: float = 120.0,
                               fade_ms: float = 5.0, max_batch: int = 8, in_flight: int = 3, pcm16: bool = False,
                               prefix_tokens: Optional[Sequence[int]] = None, trim=None, align=None, return_words: bool = False,
                               return_pieces: bool = False, takes=None, repair=None, deliver=None,
                               batch_sizes: Optional[Sequence[int]] = (1, 2, 4, 8), watermark=None, retime=None):
        """synthesize_long handed out batch by batch: a generator of LongChunk(audio, index, offset, segments, words,
        pieces), one per group of pieces, whose audio concatenated along axis 1 is the joined waveform.  The arguments are
        synthesize_long's (without the return_takes / return_repair reports; the segments always come, in the chunks).

        `batch_sizes`: the pieces ride in stream_groups(pieces, batch_sizes, max_batch): by default one piece first, then 2, 4, 8,
        8, ..., so that the first chunk leaves after one small batch; None: plan_long's groups, and then the chunks' concatenation
        IS synthesize_long(...)'s waveform for the same arguments, bit for bit, and the concatenated segments, words and pieces
        equal its lists (another grouping changes batch shapes: equal within the engine's batch-shape tolerance).

        Up to `in_flight` groups are enqueued ahead, each on its own stream and workspace under throughput tuning, as synthesize_long
        enqueues them; the tuning and the workspace are the caller's again before every yield.  When a group's batch has completed
        and the fp16 range guard has been read (engine.check_fp16_range(in_flight=True): no device-wide wait), its tail goes onto
        the caller's stream: engine.join_stream appends its pieces to the joined stream, planned on the device from the table
        engine.endpoints left there, then engine.deliver_from_table when `deliver` is given (one delivery stream for the whole text:
        the chunks continue each other as DecodeStream's do), then ONE pinned copy of the audio with the positions and whatever the
        flags asked for.  The host waits once, enqueues the next group and yields.  If the guard demotes a site, chunks already
        handed out stay; the groups in flight are waited for and run again one at a time, in order, and the rest of the text runs at
        the demoted precision.  With `deliver`, offsets, segments and words are in output samples by synthesize_long's rule; a
        chunk's `offset` is the count of samples handed out before it (the resampler's look-ahead moves a little audio from one
        chunk into the next; the last chunk flushes).

        Closing the generator early waits for what is in flight and leaves the engine as a finished call does.  Empty text yields
        nothing.  Arguments are checked here, before the first next().  `retime` is refused: a chain's state is not carried across
        chunks; retime the whole text with synthesize_long."""
        if retime is not None:
            raise ValueError("synthesize_long_stream: retime= is not streamed (no chain state is carried across chunks): use "
                             "synthesize_long(retime=)")
        q = self._long_request("synthesize_long_stream", voice, text, token_lists, durations, prefix_tokens, max_batch, pcm16, trim,
                               align, return_words, takes, repair, deliver, watermark)
        toks, ns = q.toks, q.ns
        groups = stream_groups(len(toks), batch_sizes, q.max_batch)
        if int(in_flight) < 1:
            raise ValueError("synthesize_long_stream: in_flight must be at least 1")
        base = (self._next_seed() if seed is None else int(seed)) if toks else 0
        seeds = [piece_seed(base, i) for i in range(len(toks))]
        calls, _al_b = self._long_calls(voice, toks, ns, seeds, groups, len(q.prefix), q.ep, q.al, q.tk, q.rp, False)
        return self._long_chunks(calls, groups, toks, ns, seeds, len(q.prefix), q.ep, int(in_flight), gap_ms, fade_ms, pcm16, q.dv,
                                 return_words, return_pieces, q.wm)

    def _long_chunks(self, calls, groups, toks, ns, seeds, n_prefix: int, ep: Optional["Endpointing"], in_flight: int,
                     gap_ms: float, fade_ms: float, pcm16: bool, dv: Optional["Delivery"], return_words: bool, return_pieces: bool,
                     wm: Optional["Watermark"] = None):
        """synthesize_long_stream's generator: the groups' deferred batches `calls`, enqueued ahead, verified, joined and handed out."""
        if not calls:
            return
        from .audio import deliver_counts
        eng = self.engine
        dev = eng.device
        cur = torch.cuda.current_stream(dev)
        L = max(1, min(in_flight, len(calls)))
        streams = [torch.cuda.Stream(dev) for _ in range(L)]
        for st in streams:
            st.wait_stream(cur)
        gap = max(0, int(round(gap_ms * SAMPLE_RATE / 1000.0)))
        w = fade_table(fade_ms)
        fade = torch.from_numpy(w).to(dev) if w.size else None
        jstate = eng.join_state()
        bank_rate = dv is not None and dv.ratio != (1, 1)
        dstate = eng.deliver_state(1, dv.rate) if bank_rate else None
        mstate = eng.watermark_state(1) if wm is not None else None   # the mark's slot: only verified batches ever advance it
        if bank_rate:
            _bank, up, down, width, _klen = eng.deliver_bank(dv.rate)
        queue: Dict[int, list] = {}                            # group -> [record, its event (None: run again on the caller's stream)]

        def enqueue(i: int) -> None:
            # throughput tuning and the named workspace around this one enqueue, _run_in_flight's: never held across a yield
            with self._throughput(), self._in_flight_slot(streams[i % L], i % L):
                rec = calls[i]()
                ev = torch.cuda.Event()
                ev.record()
            queue[i] = [rec, ev]

        def tail(gi: int, rec: _Batch):
            """Group gi's join, delivery and ONE copy out, on the caller's stream -> (host bytes, the layout to read them by)."""
            g = groups[gi]
            if ep is None:
                seg, gain = eng._upload_i64([[0, HOP_SIZE * n] for n in rec.ns]), None
            else:
                seg, gain = rec.seg, (rec.gain if ep.level_dbfs is not None else None)
            cap = sum(HOP_SIZE * n for n in rec.ns) + len(g) * gap       # no window is longer than its row's hop * n samples
            last = gi == len(groups) - 1
            chunk, off, pos, dtable = eng.join_stream(rec.audio, seg, gain, fade, gap, jstate, last=last, pcm16=pcm16, cap=cap,
                                                      deliver_slot=0)
            audio = chunk if dv is None else eng.deliver_from_table(chunk, dtable, dv.rate, dv.encoding, state=dstate, mark=wm,
                                                                    mark_state=mstate)
            parts = [("off", off), ("pos", pos)]
            if ep is not None:
                parts += [("seg", rec.seg), ("gain", rec.gain)]
            if return_words:
                parts.append(("spans", rec.spans))
            if return_pieces:
                parts.append(("latents", rec.latents))
                if rec.winner is not None:
                    parts.append(("winner", rec.winner))
            parts.append(("audio", audio))                     # 8-byte items first, the audio last: every part starts aligned
            packed = torch.cat([t.reshape(-1).view(torch.uint8) for _name, t in parts])
            host = torch.empty(packed.numel(), dtype=torch.uint8, pin_memory=True)
            host.copy_(packed, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            done.synchronize()                                 # the one wait of the tail
            flat, res, at = host.numpy().copy(), {}, 0
            for name, t in parts:
                nb = t.numel() * t.element_size()
                res[name] = flat[at: at + nb].view(_NP_OF[t.dtype]).reshape(tuple(t.shape))
                at += nb
            return res, last

        n_words, sent, nxt = 0, 0, 0
        try:
            while nxt < L:
                enqueue(nxt)
                nxt += 1
            for gi, g in enumerate(groups):
                rec, ev = queue[gi]
                with torch.cuda.stream(cur):                   # (the consumer may have changed streams between two chunks)
                    if ev is not None:
                        ev.synchronize()
                        if eng.check_fp16_range("synthesize_long_stream", in_flight=True):
                            # clipped somewhere: what was handed out stays; everything enqueued and not handed out again, one at a time,
                            # in order, on the caller's stream at the demoted precision (the joined stream only ever advances by
                            # verified batches)
                            for st in streams:
                                st.synchronize()
                            eng.check_fp16_range("synthesize_long_stream")   # all of it has finished: the counters start from zero again
                            for j in sorted(queue):
                                queue[j] = [queue[j][0].rerun(), None]
                            rec = queue[gi][0]
                        else:
                            cur.wait_event(ev)
                    res, last = tail(gi, rec)
                del queue[gi]
                if nxt < len(calls):
                    enqueue(nxt)
                    nxt += 1
                pos0, pos1 = int(res["pos"][0]), int(res["pos"][1])
                count = pos1 - pos0 if not bank_rate else deliver_counts(pos0, pos1 - pos0, last, up, down, width)
                audio = res["audio"].reshape(1, -1)[:, :count]
                segs, words, made = _piece_rows(res["off"], res.get("seg"), res.get("gain"), res.get("spans"), res.get("latents"),
                                                res.get("winner"), [toks[i] for i in g], [ns[i] for i in g], [seeds[i] for i in g],
                                                n_prefix, ep, return_words, return_pieces, n_words)
                n_words += len(words or ())
                segs, words = _to_output_samples(dv, segs, words)   # synthesize_long's rule
                chunk = LongChunk(audio, gi, pos0 if dv is None else sent, segs, words, made)
                sent += count
                yield chunk
        finally:
            # a consumer that stopped listening, an error, or the end: wait for what is in flight and leave the engine as a finished
            # call does (the tuning and the workspace are the caller's already: they are never held across a yield)
            queue.clear()
            for st in streams:
                st.synchronize()
                cur.wait_stream(st)
            eng.check_fp16_range("synthesize_long_stream")

    def render_long(self, pieces, *, gap_ms: float = 120.0, fade_ms: float = 5.0, max_batch: int = 8, in_flight: int = 3,
                    pcm16: bool = False, trim=None, return_segments: bool = False, retime=None):
        """The decode, endpoints and join half of synthesize_long for given latents: `pieces` are Pieces
        (synthesize_long(return_pieces=True)) or (n_i, 64) arrays, in order.  They are grouped as plan_long groups them, decoded
        through the same in-flight machinery under the same tuning and joined by the same kernels, so that the pieces of a take,
        rendered with the take's parameters, give the take's waveform again bit for bit; with one piece replaced by a re-spoken
        one of the same length every other piece's segment stays as it was (the decoder is causal and rows do not see each other).
        A replacement of another length changes the shape of its group's batch: the other rows of that group then agree within the
        engine's batch-shape tolerance, not bit for bit.  `retime`: synthesize_long's, on the joined row.  -> waveform (1, S)[,
        segments] as synthesize_long."""
        rt = _long_retime("render_long", retime, pcm16)
        ep = as_endpointing(trim)
        lats = _piece_latents(pieces)
        ns = [int(l.shape[0]) for l in lats]
        groups, offsets, S = plan_long(ns, max_batch, gap_ms)
        if not lats:
            empty = np.zeros((1, 0), np.int16 if pcm16 else np.float32)
            return (empty, []) if return_segments else empty
        eng = self.engine

        def decode_only(g):
            g_ns = [ns[i] for i in g]
            lat = np.zeros((len(g), max(g_ns), 64), np.float32)
            for r, i in enumerate(g):
                lat[r, : ns[i]] = lats[i]

            def run() -> _Batch:
                x = torch.from_numpy(lat).to(eng.device)
                audio = eng.codec_decode(x)
                seg, gain = eng.endpoints(audio, g_ns, ep)[:2] if ep is not None else (None, None)
                return _Batch(audio, x, None, None, seg, gain, g_ns, run)
            return run

        out, segs, _pending, table = self._join_long([decode_only(g) for g in groups], groups, ns, offsets, S, ep, in_flight, gap_ms,
                                                     fade_ms, pcm16, rt=rt)
        if table is not None:
            segs = _retimed_segments(segs, table)
        return (out, segs) if return_segments else out

    def respeak(self, tokens: Sequence[int], latents, frames: Tuple[int, int], *, voice: Optional[Voice] = None, ref_latents=None,
                new_tokens: Optional[Sequence[int]] = None, new_frames: Optional[int] = None, seed: Optional[int] = None,
                start_step: int = 0, trim=None, align=None, prefix_len: int = 0, return_alignment: bool = False, takes=None,
                return_takes: bool = False):
        """Speaks frames [f0, f1) = `frames` of one utterance again and keeps the rest: `latents` (n, 64) are the utterance's (from
        return_latents / a Piece), `tokens` its token list; one row through synthesize_batch(pins=splice_pins(latents, f0, f1,
        new_frames)).  -> (audio (1, S'), latents (n', 64)[, words with align=]), n' = n - (f1 - f0) + new_frames: the frames in front
        of f0 and behind f1 come back bit for bit (the tail at its shifted place), and so does the audio in front of sample
        3200 * f0 when the row is decoded in a batch of the same shape (the codec is causal).  Which frames speak a word:
        frames_of_groups on the spans of align=.

        `new_tokens`: the row's WHOLE new token list when the text changes (default: `tokens`); `new_frames`: the length of the
        regenerated region (default f1 - f0).  `voice` or `ref_latents`: the reference, one of them.  `seed`: the noise of the new
        take — a new take needs a new seed: with the seed the row was first spoken with, the free frames see much the same noise
        again.  None draws one.  `start_step` = k > 0 runs only the sampler steps from k on, from `latents` themselves in the
        free region too (same length only); start_step = num_steps - 1 is nearly a no-op by the schedule (alpha(0) = 1,
        sigma(0) = 3.1e-5).  `prefix_len`: leading tokens that are a prepended transcription (align= leaves them out).
        `return_alignment` (with align=): one more element, (mass (n', P) fp32, spans (P, 2) int32) of the new row.
        `takes` / `return_takes`: as synthesize_batch's; the row is re-spoken K times from take_seed(seed, k), every take with the
        same pins, and the best-aligned one comes back (with return_takes one more element at the end: (winner k, the winner's
        seed, totals, features)).

        Only the mechanism is verified.  It is UNVALIDATED on trained weights: every weight this project has run is seeded noise,
        and nobody has measured how well a 4-step distilled student inpaints."""
        if (voice is None) == (ref_latents is None):
            raise ValueError("respeak: pass either voice or ref_latents")
        if not isinstance(frames, (tuple, list)) or len(frames) != 2:
            raise ValueError("respeak: frames must be (f0, f1)")
        f0, f1 = int(frames[0]), int(frames[1])
        x_pin, keep = splice_pins(latents, f0, f1, new_frames)
        start_step = int(start_step)
        if start_step > 0:
            if x_pin.shape[0] != np.asarray(latents).shape[0]:
                raise ValueError("respeak: start_step > 0 starts from the given latents: new_frames must equal f1 - f0")
            x_pin[f0:f1] = np.asarray(latents, np.float32)[f0:f1]
        toks = [int(t) for t in (tokens if new_tokens is None else new_tokens)]
        if not 0 <= int(prefix_len) <= len(toks):
            raise ValueError("respeak: prefix_len must lie in [0, number of tokens]")
        al = as_alignment(align)
        if return_alignment and al is None:
            raise ValueError("respeak: return_alignment= belongs to align=")
        tk = as_takes(takes)
        scored = tk is not None and (tk.k > 1 or return_takes)   # synthesize_batch's rule: these takes are aligned, so the prefix counts
        res = self.synthesize_batch(None if voice is not None else [np.asarray(ref_latents, np.float32)], [toks], None,
                                    frames=[int(x_pin.shape[0])], voices=None if voice is None else [voice],
                                    seeds=[self._next_seed() if seed is None else int(seed)], trim=trim, return_latents=True,
                                    pins=[(x_pin, keep)], start_step=start_step, takes=tk, return_takes=bool(return_takes),
                                    **({} if al is None and not scored else {"prefix_lens": [int(prefix_len)]}),
                                    **({} if al is None else {"align": al, "return_alignment": bool(return_alignment)}))
        return (res[0][0], res[1][0]) + tuple(r[0] for r in res[2:])   # (words, raw alignment and takes: only when asked for)

    def synthesize_sharded(self, ref_latents: Sequence[np.ndarray], phoneme_ids: Sequence[Sequence[int]],
                           duration_sec: float, *, max_batch: int = 8) -> np.ndarray:
        """Data-parallel synthesis of a request list with a common duration -> (n, 1, samples) fp32 on the host.

        * under torch.distributed (one process per GPU, e.g. `python -m torch.distributed.run --nproc-per-node 8`): every rank
          passes the same list, synthesises its contiguous shard and receives the whole batch after ONE RCCL all-gather
          (`smalltts_amd.parallel.ShardContext`; the configuration `bench.py --gpus N` measures);
        * otherwise over `device_ids` from this process (one engine + one host thread per GPU, gathered on the host);
        * with one GPU: plain batches of `max_batch`."""
        from . import parallel
        n = len(ref_latents)
        S = _frames(duration_sec) * HOP_SIZE

        def run_span(tts: "SmallTTS", lo: int, hi: int) -> list:
            outs: list = []
            with torch.cuda.device(tts.engine.device):
                for s0 in range(lo, hi, max_batch):
                    s1 = min(hi, s0 + max_batch)
                    outs.extend(tts.synthesize_batch(list(ref_latents[s0:s1]), list(phoneme_ids[s0:s1]), duration_sec))
            return outs

        ctx = parallel.ShardContext.current()
        if ctx.world > 1:
            full = parallel.synthesize_sharded(lambda r, p, d: run_span(self, *ctx.my_shard(n)), ref_latents, phoneme_ids,
                                               duration_sec, ctx=ctx)
            return full.cpu().numpy()
        if len(self._replicas) > 1:
            outs = parallel.run_shards_in_threads([lambda lo, hi, t=t: run_span(t, lo, hi) for t in self._replicas], n)
        else:
            outs = run_span(self, 0, n)
        return np.stack(outs) if outs else np.zeros((0, 1, S), np.float32)

    def synthesize(self, ref_latents: np.ndarray, phoneme_ids: list, duration_sec: float) -> np.ndarray:
        """ref_latents (T,64) f32, phoneme ids, duration -> audio (1, samples) f32 @ 24 kHz."""
        return self.synthesize_batch([ref_latents], [phoneme_ids], [duration_sec])[0]

    def synthesize_stream(self, ref_latents: Optional[np.ndarray], phoneme_ids: Sequence[int], duration_sec: float, *,
                          chunk_frames: Sequence[int] = (2, 4, 8, 16, 32), pcm16: bool = False, seed: Optional[int] = None,
                          voice: Optional[Voice] = None, frames: Optional[int] = None, return_latents: bool = False, deliver=None,
                          watermark=None):
        """synthesize() that hands the audio out while it is still being decoded: -> an iterator of numpy chunks
        (1, samples) fp32, or int16 with pcm16=True (engine.pcm16 on the device), whose concatenation is the utterance.
        The sampler runs ONCE, exactly as synthesize_batch runs it for this row (same seeds: `seed` is its seeds=[seed]; same
        latents bit for bit; same fp16 range guard on the DiT sites), on the call; the latents are then decoded in chunks of
        chunk_frames[0], chunk_frames[1], ... frames (stream_chunks: the last size repeats, the final chunk is what is left)
        through engine.codec_decode_stream, whose carried state makes the chunks continue each other.  Per chunk: one D2D copy of
        the state slot (the snapshot a re-decode starts from), the decode, the copy into one of two alternating pinned host
        buffers and an event.  The event is waited for and the fp16 range counters are read before the chunk is yielded; a codec
        site that clamped is demoted (engine.check_fp16_range) and that chunk alone is decoded again from its snapshot; a DiT site
        that clamped (seen at the first chunk) runs the sampler again.  Reading the counters synchronises the device, so chunk
        k + 1 is enqueued right behind that read and in front of the yield of chunk k: the device decodes chunk k + 1 while the
        caller consumes chunk k, and no chunk waits for the decode of its successor.  `voice` (encode_voice) instead of
        ref_latents (pass None); `frames` overrides floor(duration * 7.5); return_latents: yields (chunk, latents (n, 64)).
        `deliver` (a Delivery, a rate or a (rate, encoding) pair): every decoded chunk is resampled and encoded on the
        device behind its decode (engine.deliver with one delivery slot next to the decode slot, last=True on the final chunk);
        the chunks are (1, count) arrays in the encoding's dtype whose sizes follow audio.deliver_counts (a chunk waits for the
        resampler's look-ahead, the final chunk flushes it) and whose concatenation is the delivery of the whole utterance, bit for
        bit.  The delivery slot is snapshotted and restored with the decode slot for a re-decode.  Not together with pcm16=True.
        `watermark` (a Watermark, a key or a (key, strength) pair): every chunk is marked in front of its delivery through
        one mark slot, snapshotted and restored with the others; the chunks concatenate to the marked utterance, bit for bit.
        Without `deliver` it means Delivery(24000, "f32").  24 kHz, f32 or pcm16 only.
        Not for trim=, align=, takes=, repair= (they need the whole utterance) or synthesize_long."""
        wm, dv = marked_delivery("synthesize_stream", watermark, as_delivery(deliver))
        if dv is not None and pcm16:
            raise ValueError("synthesize_stream: deliver= (and with it watermark=) and pcm16=True exclude each other: ask for "
                             "Delivery(rate, 'pcm16')")
        sizes_in = [int(c) for c in chunk_frames]
        if not sizes_in or min(sizes_in) < 1:
            raise ValueError("synthesize_stream: chunk_frames needs at least one size, all >= 1")
        if (voice is None) == (ref_latents is None):
            raise ValueError("synthesize_stream: pass either ref_latents or voice (with ref_latents=None)")
        rec = self.synthesize_batch(None if voice is not None else [ref_latents], [phoneme_ids], [duration_sec],
                                    frames=None if frames is None else [int(frames)], seeds=None if seed is None else [int(seed)],
                                    voices=None if voice is None else [voice], _defer=True, _decode=False)
        return self._stream_chunks(rec, stream_chunks(rec.ns[0], sizes_in), bool(pcm16), bool(return_latents), dv, wm)

    def _stream_chunks(self, rec: _Batch, sizes: Sequence[int], pcm16: bool, return_latents: bool, dv: Optional["Delivery"] = None,
                       wm: Optional["Watermark"] = None):
        eng = self.engine
        if not sizes:
            return
        state = eng.decode_state(1)
        snap = torch.empty_like(state)
        dt = torch.int16 if pcm16 else torch.float32
        hop = eng.hop                                          # (the loaded codec's, not the reference constant: test specs differ)
        cnt = [hop * c for c in sizes]                         # samples chunk k hands out
        dstate = dsnap = None
        mstate = None if wm is None else eng.watermark_state(1)   # the mark's slot, next to the decode slot (24 kHz: dstate is None)
        msnap = None if wm is None else torch.empty_like(mstate)
        if dv is not None:                                     # one delivery slot next to the decode slot; sizes from integers alone
            from .audio import deliver_counts
            _bank, up, down, width, _klen = eng.deliver_bank(dv.rate)
            dt = torch.from_numpy(np.zeros(0, dv.dtype)).dtype
            dstate = eng.deliver_state(1, dv.rate)             # None at 24 kHz: a pure encode carries nothing
            dsnap = None if dstate is None else torch.empty_like(dstate)
            if dstate is not None:
                t0s = np.concatenate([[0], np.cumsum(sizes)[:-1]])
                cnt = [deliver_counts(hop * int(t), hop * c, k == len(sizes) - 1, up, down, width) for k, (t, c) in enumerate(zip(t0s, sizes))]
        host = [torch.empty(1, max(max(cnt), 1), dtype=dt).pin_memory() for _ in range(2)]

        def deliver_kw(k: int, t0: int) -> dict:
            """How chunk k is delivered: through the resampler's slot, or (24 kHz, a pure encode without state) the mark's, or neither."""
            if dstate is not None:
                return {"state": dstate, "slots": [0], "n_before": [hop * t0], "last": k == len(sizes) - 1}
            if wm is not None:
                return {"slots": [0], "n_before": [hop * t0], "mark": wm, "mark_state": mstate}
            return {}

        def enqueue(k: int, t0: int):
            snap.copy_(state)                                  # what a re-decode of chunk k starts from
            a = eng.codec_decode_stream(rec.latents[:, t0:t0 + sizes[k]], state, [0])
            if dv is not None:
                if dstate is not None:
                    dsnap.copy_(dstate)
                elif wm is not None:
                    msnap.copy_(mstate)
                a = eng.deliver(a, [hop * sizes[k]], dv.rate, dv.encoding, **deliver_kw(k, t0))[0][None]
            a = eng.pcm16(a) if pcm16 else a
            host[k % 2][:, :cnt[k]].copy_(a[0][:, :cnt[k]], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            return ev
        ev, t0, lat = enqueue(0, 0), 0, None
        for k, c in enumerate(sizes):
            ev.synchronize()
            for _ in range(len(SITES) + 1):                    # every pass demotes a site: it ends
                hit = eng.check_fp16_range("synthesize_stream")
                if not hit:
                    break
                if any(not str(site).startswith("codec") for site in hit):   # the latents were clipped: sample again, start over
                    assert k == 0, "a DiT site clamped behind the sampler"
                    rec = rec.rerun()
                state.copy_(snap)
                if dstate is not None:
                    dstate.copy_(dsnap)
                if mstate is not None:
                    mstate.copy_(msnap)
                ev = enqueue(k, t0)
                ev.synchronize()
            out = host[k % 2][:, :cnt[k]].numpy().copy()
            if return_latents and lat is None:
                lat = rec.latents[0].cpu().numpy()
            if k + 1 < len(sizes):
                ev = enqueue(k + 1, t0 + c)
            yield (out, lat[t0:t0 + c]) if return_latents else out
            t0 += c

    def forward(self, conditionings: List[torch.Tensor], transcriptions: list, texts: list,
                duration_sec: float = 3.0) -> List[torch.Tensor]:
        from .phonemes import get_token_ids
        toks = []
        for trans, text in zip(transcriptions, texts):
            a = get_token_ids(trans) if isinstance(trans, str) else list(map(int, trans))
            b = get_token_ids(text) if isinstance(text, str) else list(map(int, text))
            toks.append(a + b)                                 # transcription + text, infer/onnx.py:144-152
        n = min(len(conditionings), len(toks))
        refs = [c.detach().cpu().numpy().astype(np.float32) for c in conditionings[:n]]
        outs = self.synthesize_batch(refs, toks[:n], duration_sec)
        return [torch.from_numpy(np.ascontiguousarray(o)) for o in outs]

    __call__ = forward


class _CodecRunner:
    _part = ""

    def __init__(self, path: str, providers: Optional[Iterable[str]] = None, *, weights: Optional[str] = None,
                 device: int = 0, precision: str = DEFAULT_PRECISION, engine: Optional[HipEngine] = None) -> None:
        self.engine = engine or get_engine(weights, device, precision, parts=("dit", "decoder", "encoder"))
        if not self.engine.has(self._part):
            raise RuntimeError(f"codec {self._part} weights are not loaded")


class Decoder(_CodecRunner):
    _part = "decoder"

    def __init__(self, path: str = "assets/codec/decoder.onnx", providers: Optional[Iterable[str]] = None, **kw):
        super().__init__(path, providers, **kw)

    def decode(self, latents: torch.Tensor) -> torch.Tensor:
        """latents f32 (batch, T, 64) -> audio f32 (batch, 1, 3200*T), returned on the CPU like the reference."""
        return self.engine.codec_decode(latents.detach()).cpu()

    def open_stream(self, rows: int = 1, deliver=None, watermark=None) -> "DecodeStream":
        """`rows` utterances decoded chunk by chunk: DecodeStream.decode(latents_chunk) continues where the last call ended.
        `deliver` (a Delivery, a rate or a (rate, encoding) pair): the chunks leave at that rate and encoding.
        `watermark` (a Watermark, a key or a (key, strength) pair): every row's stream is marked in front of the delivery."""
        return DecodeStream(self.engine, rows, deliver, watermark)


class DecodeStream:
    """The causal state of `rows` utterances being decoded in chunks (engine.codec_decode_stream).  decode(chunk (rows, T, 64)) ->
    audio (rows, 1, 3200 * T) on the CPU; the concatenated chunks are Decoder.decode of the concatenated latents.  reset(): all rows
    start a new utterance.  snapshot() / restore(s): rewind to a point between two chunks.
    With `deliver` decode(chunk, last=False) -> (rows, count) on the CPU in the Delivery's dtype: the chunk at its rate and
    encoding, count = audio.deliver_counts of the samples seen so far (the resampler's look-ahead is held back until last=True
    flushes it); the concatenated chunks are engine.deliver of the whole decode, bit for bit.  The delivery slots are reset,
    snapshotted and restored together with the decode slots.
    With `watermark` (24 kHz, f32 or pcm16, Delivery(24000, "f32") without `deliver`) every row is marked as one stream in
    front of the delivery; the mark slots are reset, snapshotted and restored with the others."""

    def __init__(self, engine: HipEngine, rows: int = 1, deliver=None, watermark=None) -> None:
        self.watermark, self.deliver = marked_delivery("DecodeStream", watermark, as_delivery(deliver))
        self.engine, self.rows = engine, int(rows)
        self.state = engine.decode_state(self.rows)
        self._slots = list(range(self.rows))
        self._dstate = None if self.deliver is None else engine.deliver_state(self.rows, self.deliver.rate)
        self._mstate = None if self.watermark is None else engine.watermark_state(self.rows)
        self._seen = 0                                         # samples every row's delivery stream has taken in

    def decode(self, latents: torch.Tensor, last: bool = False) -> torch.Tensor:
        if latents.dim() != 3 or int(latents.shape[0]) != self.rows:
            raise ValueError(f"DecodeStream.decode: a ({self.rows}, T, 64) chunk wanted, got {tuple(latents.shape)}")
        audio = self.engine.codec_decode_stream(latents.detach(), self.state, self._slots)
        if self.deliver is None:
            return audio.cpu()
        n = int(audio.shape[-1])
        kw = {} if self._dstate is None else {"state": self._dstate, "slots": self._slots, "n_before": [self._seen] * self.rows,
                                              "last": bool(last)}
        if self._mstate is not None:                           # (24 kHz: no delivery state, the mark's slots alone)
            kw = {"slots": self._slots, "n_before": [self._seen] * self.rows, "mark": self.watermark, "mark_state": self._mstate}
        out, counts = self.engine.deliver(audio, [n] * self.rows, self.deliver.rate, self.deliver.encoding, **kw)
        self._seen += n
        return out[:, :counts[0]].cpu()

    def reset(self) -> None:
        self.state.zero_()
        if self._dstate is not None:
            self._dstate.zero_()
        if self._mstate is not None:
            self._mstate.zero_()
        self._seen = 0

    def snapshot(self):
        if self.deliver is None:
            return self.state.clone()
        return (self.state.clone(), None if self._dstate is None else self._dstate.clone(), self._seen,
                None if self._mstate is None else self._mstate.clone())

    def restore(self, snap) -> None:
        if self.deliver is None:
            self.state.copy_(snap)
            return
        self.state.copy_(snap[0])
        if self._dstate is not None:
            self._dstate.copy_(snap[1])
        if self._mstate is not None:
            self._mstate.copy_(snap[3])
        self._seen = int(snap[2])


class Encoder(_CodecRunner):
    _part = "encoder"

    def __init__(self, path: str = "assets/codec/encoder.onnx", providers: Optional[Iterable[str]] = None, **kw):
        super().__init__(path, providers, **kw)

    def encode(self, audio: torch.Tensor) -> torch.Tensor:
        """audio f32 (batch, 1, time) @ 24 kHz -> latents f32 (batch, time // 3200, 64), on the CPU."""
        return self.engine.codec_encode(audio.detach()).cpu()

    # reference voices are encoded once per voice (clone.py:36, interactive.py:34): latents cached by content hash
    _ref_cache: "collections.OrderedDict[bytes, torch.Tensor]" = None  # type: ignore[assignment]
    REF_CACHE_ENTRIES = 64

    def encode_reference(self, audio: torch.Tensor) -> torch.Tensor:
        """Like encode() for ONE reference clip (1, 1, time), memoised on the samples' digest."""
        if Encoder._ref_cache is None:
            Encoder._ref_cache = collections.OrderedDict()
        a = audio.detach().to(torch.float32).contiguous().cpu()
        key = hashlib.blake2b(a.numpy().tobytes(), digest_size=16, person=str(tuple(a.shape)).encode()[:16]).digest()
        key += str(id(self.engine)).encode()
        hit = Encoder._ref_cache.get(key)
        if hit is not None:
            Encoder._ref_cache.move_to_end(key)
            return hit
        lat = self.encode(a)
        Encoder._ref_cache[key] = lat
        while len(Encoder._ref_cache) > self.REF_CACHE_ENTRIES:
            Encoder._ref_cache.popitem(last=False)
        return lat
