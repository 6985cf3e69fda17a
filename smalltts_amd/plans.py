"""The pure host arithmetic of the synthesis calls (api.py): text splitting, join and stream plans, token groups and word timings,
pins, seeds.  numpy only: nothing here touches the device or imports torch."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

SAMPLE_RATE = 24_000
HOP_SIZE = 3_200
NUM_STEPS = 4
CHARS_PER_SECOND = 11.5


def estimate_duration(text: str, min_sec: float = 0.5, max_sec: float = 30.0) -> float:
    return max(min_sec, min(len(text) / CHARS_PER_SECOND, max_sec))


def _frames(duration_sec: float) -> int:
    return max(1, int(duration_sec * SAMPLE_RATE / HOP_SIZE))  # floor, infer/onnx.py:84


# ---- long-form text: pieces the model was trained for (5 - 198 phonemes, at most ~30 s per utterance) --------------------------
_SENTENCE_END = ".!?…"
_CLAUSE_END = ";:,—"


def _default_count_tokens(s: str) -> int:
    from .phonemes import get_token_ids
    return len(get_token_ids(s))


def _hard_cut(word: str, fits: Callable[[str], bool]) -> List[str]:
    """A single whitespace-free run that is over budget: longest fitting prefixes, never ending inside an `[event]` tag."""
    from .phonemes import _EVENT_RE
    out = []
    while word and not fits(word):
        tags = [m.span() for m in _EVENT_RE.finditer(word)]
        cut = 0
        for n in range(len(word) - 1, 0, -1):
            if any(a < n < b for a, b in tags):
                continue
            if fits(word[:n]):
                cut = n
                break
        if cut == 0:
            raise ValueError(f"split_text: the budgets do not admit even one character or [event] tag of {word[:24]!r}")
        out.append(word[:cut])
        word = word[cut:]
    if word:
        out.append(word)
    return out


def split_text(text: str, max_tokens: int = 198, max_seconds: float = 30.0,
               count_tokens: Optional[Callable[[str], int]] = None) -> List[str]:
    """Cuts a text into pieces that each fit one utterance: `count_tokens(piece) <= max_tokens` and
    `len(piece) / CHARS_PER_SECOND <= max_seconds` (estimate_duration without its clamp).  Cuts prefer sentence ends (`.!?…` in
    front of whitespace or the end), then clause punctuation (`;:,—`), then whitespace; only a whitespace-free run that is over
    budget on its own is cut inside, and never inside an `[event]` tag.  Greedy: a piece is extended while the next unit still
    fits, so short sentences share a piece.  " ".join(pieces) is the text with runs of whitespace collapsed (up to hard cuts).
    `count_tokens` defaults to len(phonemes.get_token_ids(s)), which needs espeak."""
    count = count_tokens or _default_count_tokens

    def fits(s: str) -> bool:
        return len(s) / CHARS_PER_SECOND <= max_seconds and count(s) <= max_tokens

    def pack(units: List[List[str]], level: int) -> List[List[str]]:
        """units: runs of words that end at a boundary of `level` (0 sentence, 1 clause, 2 word).  Greedy in-order packing; a unit
        that does not fit on its own is split at the next weaker boundary."""
        pieces: List[List[str]] = []
        cur: List[str] = []
        for u in units:
            if cur and fits(" ".join(cur + u)):
                cur = cur + u
                continue
            if cur:
                pieces.append(cur)
                cur = []
            if fits(" ".join(u)):
                cur = u
            elif level < 2:
                sub = pack(_units(u, level + 1), level + 1)
                pieces.extend(sub[:-1])
                cur = sub[-1]        # the tail may still take what follows
            else:                    # one word over budget
                sub = [[w] for w in _hard_cut(u[0], fits)]
                pieces.extend(sub[:-1])
                cur = sub[-1]
        if cur:
            pieces.append(cur)
        return pieces

    words = text.split()   # an `[event]` tag holds no whitespace: it stays inside its word
    if not words:
        return []
    return [" ".join(p) for p in pack(_units(words, 0), 0)]


def _units(words: List[str], level: int) -> List[List[str]]:
    """Groups words into runs that end behind a word closing with sentence (level 0) / clause (level 1) punctuation, optionally
    followed by closing quotes or brackets; level 2: one word per unit."""
    if level >= 2:
        return [[w] for w in words]
    marks = _SENTENCE_END if level == 0 else _SENTENCE_END + _CLAUSE_END
    units, cur = [], []
    for w in words:
        cur.append(w)
        if w.rstrip("\"'”’»)")[-1:] in marks:
            units.append(cur)
            cur = []
    if cur:
        units.append(cur)
    return units


def fade_table(fade_ms: float) -> np.ndarray:
    """Raised-cosine fade-in weights w[i] = 0.5 - 0.5 cos(pi (i + 0.5) / F), F = round(fade_ms * 24): float64 math, rounded to fp32 once."""
    F = int(round(fade_ms * SAMPLE_RATE / 1000.0))
    if F <= 0:
        return np.zeros((0,), np.float32)
    return (0.5 - 0.5 * np.cos(np.pi * (np.arange(F, dtype=np.float64) + 0.5) / F)).astype(np.float32)


def plan_long(ns: Sequence[int], max_batch: int = 8, gap_ms: float = 120.0, hop: int = HOP_SIZE) -> Tuple[List[List[int]], List[int], int]:
    """The host-side plan of synthesize_long for pieces of `ns` frames: consecutive groups of at most `max_batch` pieces (the
    splitter bounds every piece by the model's utterance limits, so a count is the only budget needed), every piece's sample
    offset in the joined waveform, and its length S = sum(hop * n_i) + (len - 1) * round(gap_ms * 24)."""
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    gap = max(0, int(round(gap_ms * SAMPLE_RATE / 1000.0)))
    groups = [list(range(i, min(i + max_batch, len(ns)))) for i in range(0, len(ns), max_batch)]
    offsets, pos = [], 0
    for n in ns:
        offsets.append(pos)
        pos += hop * int(n) + gap
    return groups, offsets, (pos - gap if len(ns) else 0)


def plan_packed(ns_trimmed: Sequence[int], gap_ms: float = 120.0) -> Tuple[List[int], int]:
    """The plan of a trimmed join: pieces of `ns_trimmed` SAMPLES (what the endpoint kernels returned), in order.  A piece with n = 0
    takes neither room nor a gap; the others lie round(gap_ms * 24) samples apart.  -> (every piece's offset in the joined waveform
    (an empty piece: where the last non-empty one ended), S = sum(n_i) + (k - 1) gap over the k non-empty pieces; 0 when all are empty)."""
    gap = max(0, int(round(gap_ms * SAMPLE_RATE / 1000.0)))
    offsets, pos, k = [], 0, 0
    for n in ns_trimmed:
        n = int(n)
        if n < 0:
            raise ValueError("plan_packed: negative length")
        if n and k:
            pos += gap
        offsets.append(pos)
        if n:
            pos += n
            k += 1
    return offsets, pos


def stream_chunks(n: int, chunk_frames: Sequence[int] = (2, 4, 8, 16, 32)) -> List[int]:
    """The chunk sizes synthesize_stream decodes n frames in: chunk_frames in order, the last size repeated, the final chunk whatever
    is left (small chunks first: the first sample leaves early; larger ones later: fewer launches per second of audio)."""
    sizes: List[int] = []
    n, k = int(n), 0
    while n > 0:
        c = min(int(chunk_frames[min(k, len(chunk_frames) - 1)]), n)
        sizes.append(c)
        n -= c
        k += 1
    return sizes


def stream_groups(n: int, batch_sizes: Optional[Sequence[int]] = (1, 2, 4, 8), max_batch: int = 8) -> List[List[int]]:
    """The groups synthesize_long_stream speaks n pieces in: consecutive pieces, the first groups of `batch_sizes` pieces each (every
    size capped by `max_batch`), the last size repeated, the final group whatever is left (a small batch first: the first chunk
    leaves after one piece's work; full batches later: the throughput of synthesize_long).  batch_sizes=None: plan_long's groups,
    `max_batch` pieces each."""
    if max_batch < 1:
        raise ValueError("max_batch must be at least 1")
    sizes = [int(max_batch)] if batch_sizes is None else [int(s) for s in batch_sizes]
    if not sizes or min(sizes) < 1:
        raise ValueError("batch_sizes must be None or a non-empty sequence of positive sizes")
    groups: List[List[int]] = []
    i, n = 0, int(n)
    while i < n:
        c = min(sizes[min(len(groups), len(sizes) - 1)], int(max_batch), n - i)
        groups.append(list(range(i, i + c)))
        i += c
    return groups


def phoneme_error_rate(ids: Sequence[int], ref: Sequence[int]) -> float:
    """Edit distance (substitutions, insertions, deletions, each 1) between two phoneme id sequences over the length of `ref`; host
    only.  An empty `ref` gives 0.0 for an empty `ids`, +inf otherwise."""
    a, b = [int(v) for v in ids], [int(v) for v in ref]
    if not b:
        return 0.0 if not a else float("inf")
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[-1] / len(b)


def token_groups(ids: Sequence[int]) -> List[Tuple[str, str, int, int]]:
    """The units word timings are reported for: runs of token ids between the space symbol.  -> [(kind, phonemes, t0, t1), ...] in
    order, [t0, t1) the run's token indices, phonemes = decode_token_ids of them.  kind "word": a run of letter / IPA symbols;
    "punct": ONE punctuation mark (a mark glued to a word is cut off it); "event": a run of up to NV_REPEAT copies of one [event]
    id (get_token_ids writes exactly NV_REPEAT).  Spaces, padding (0) and unknown ids separate runs and belong to none."""
    from .phonemes import EVENTS, NV_REPEAT, PUNCTUATION, decode_token_ids, idx2p, p2idx
    punct = {p2idx[c] for c in PUNCTUATION if c != " "}
    events = {p2idx[f"[{e}]"] for e in EVENTS}
    ids = [int(t) for t in ids]
    out: List[Tuple[str, str, int, int]] = []
    i, n = 0, len(ids)
    while i < n:
        t = ids[i]
        if t == p2idx[" "] or t not in idx2p:
            i += 1
        elif t in punct:
            out.append(("punct", decode_token_ids(ids[i:i + 1]), i, i + 1))
            i += 1
        elif t in events:
            j = i
            while j < n and ids[j] == t and j - i < NV_REPEAT:
                j += 1
            out.append(("event", decode_token_ids(ids[i:i + 1]), i, j))
            i = j
        else:
            j = i
            while j < n and ids[j] in idx2p and ids[j] != p2idx[" "] and ids[j] not in punct and ids[j] not in events:
                j += 1
            out.append(("word", decode_token_ids(ids[i:j]), i, j))
            i = j
    return out


def word_times(groups: Sequence[Tuple[str, str, int, int]], spans, n_frames: int, *, token0: int = 0,
               window: Optional[Tuple[int, int]] = None, offset: int = 0, index0: int = 0, hop: int = HOP_SIZE) -> List[Tuple[int, str, int, int]]:
    """Token spans of one row -> [(group index, kind, start sample, end sample), ...].  spans[t] = (first, last) frame of token t
    (smtts_align_path); group g covers tokens [token0 + t0, token0 + t1): start = hop * first(t0), end = hop * (last(t1 - 1) + 1),
    both clipped to the row's hop * n_frames samples.  window = (start, n), the row's speech window (trim): the span is intersected
    with it and counted from its start.  offset: where the row (or its window) starts on the caller's timeline; index0: the first
    group's index.  A group whose tokens are not on the path (an empty row) collapses to (offset, offset)."""
    total = hop * max(0, int(n_frames))
    out = []
    for gi, (kind, _ph, t0, t1) in enumerate(groups):
        first, last = int(spans[token0 + t0][0]), int(spans[token0 + t1 - 1][1])
        if first < 0 or last < 0:
            s = e = 0
        else:
            s, e = min(hop * first, total), min(hop * (last + 1), total)
        if window is not None:
            ws, wn = int(window[0]), int(window[1])
            s, e = min(max(s - ws, 0), wn), min(max(e - ws, 0), wn)
        out.append((index0 + gi, kind, int(offset) + s, int(offset) + e))
    return out


def _srt_time(samples: int) -> str:
    ms = (int(samples) * 1000 + SAMPLE_RATE // 2) // SAMPLE_RATE
    return f"{ms // 3600000:02d}:{ms // 60000 % 60:02d}:{ms // 1000 % 60:02d},{ms % 1000:03d}"


def format_srt(cues: Sequence[Tuple[int, int, str]]) -> str:
    """[(start sample, end sample, text), ...] at 24 kHz -> the text of a SubRip file: numbered cues, times rounded to the nearest
    millisecond, an end never before its start; cues with empty text are dropped."""
    out, k = [], 0
    for s, e, text in cues:
        text = str(text).strip()
        if not text:
            continue
        k += 1
        out.append(f"{k}\n{_srt_time(s)} --> {_srt_time(max(int(s), int(e)))}\n{text}\n")
    return "\n".join(out)


def frames_of_groups(groups: Sequence[Tuple[str, str, int, int]], spans, g0: int, g1: int, token0: int = 0) -> Tuple[int, int]:
    """The frames token groups [g0, g1) of one row touch, by word_times' mapping: (first frame of the first token, last frame of the
    last token + 1).  groups: token_groups of the row's own tokens; spans[t] = (first, last) frame of token t (smtts_align_path);
    token0: the prepended tokens in front of them.  A group off the path (an empty row) raises ValueError."""
    g0, g1 = int(g0), int(g1)
    if not 0 <= g0 < g1 <= len(groups):
        raise ValueError(f"frames_of_groups: groups [{g0}, {g1}) outside [0, {len(groups)}) or empty")
    t0, t1 = int(groups[g0][2]), int(groups[g1 - 1][3])
    if token0 + t0 < 0 or token0 + t1 > len(spans):
        raise ValueError(f"frames_of_groups: tokens [{token0 + t0}, {token0 + t1}) outside the span table of {len(spans)} tokens")
    first, last = int(spans[token0 + t0][0]), int(spans[token0 + t1 - 1][1])
    if first < 0 or last < first:
        raise ValueError(f"frames_of_groups: groups [{g0}, {g1}) are not on the alignment path")
    return first, last + 1


CTC_FRAMES_PER_CODEC_FRAME = 4                    # the recogniser runs at 4 frames per latent frame (engine.ASR_UPSAMPLE)
CTC_HOP = HOP_SIZE // CTC_FRAMES_PER_CODEC_FRAME  # 800 samples, 33.3 ms: the resolution of a CTC alignment


LONG_WINDOW, LONG_HOP = 225, 180                  # asr_logprobs_long: latent frames per recogniser window, and between window starts


def long_windows(N: int) -> Tuple[List[int], List[int], np.ndarray]:
    """The window table of engine.asr_logprobs_long for a recording of N latent frames -> (starts a_w, cuts c_0 .. c_{n_w},
    src int32 (N,): the window of every frame).  N <= 225: one window [0, N).  Else n_w = 1 + ceil((N - 225) / 180) full windows,
    a_w = min(180 w, N - 225); c_0 = 0, c_{n_w} = N, c_w = (a_{w-1} + 225 + a_w) // 2, the midpoint of the overlap of windows w - 1
    and w: frame n in [c_w, c_{w+1}) comes from window w, at local frame n - a_w."""
    N = int(N)
    if N < 1:
        raise ValueError(f"long_windows: N = {N} must be at least 1")
    if N <= LONG_WINDOW:
        return [0], [0, N], np.zeros((N,), np.int32)
    n_w = 1 + -(-(N - LONG_WINDOW) // LONG_HOP)
    starts = [min(w * LONG_HOP, N - LONG_WINDOW) for w in range(n_w)]
    cuts = [0] + [(starts[w - 1] + LONG_WINDOW + starts[w]) // 2 for w in range(1, n_w)] + [N]
    src = np.repeat(np.arange(n_w, dtype=np.int32), np.diff(np.asarray(cuts, np.int64)))
    return starts, cuts, src


def encoder_lookback(kernel: int, enc_ratios: Sequence[int], enc_depths: Sequence[int]) -> int:
    """Samples of audio in front of a codec frame's own hop that the causal encoder reads for it (weights.CodecSpec: stem conv, per
    stage a strided conv of kernel 2 r behind the first and `depth` blocks of one depthwise conv each, head conv; every conv padded
    on the left by kernel - stride).  A conv whose input sits every j samples looks (kernel - stride) j samples back.  The default
    codec: 185 562 samples, 58 codec frames (what align_wav_long's enc_context is measured against)."""
    k, j = int(kernel), 1
    back = (k - 1) * j + int(enc_depths[0]) * (k - 1) * j       # stem, stage 0
    for r, depth in zip(enc_ratios, enc_depths[1:]):
        back += int(r) * j                                      # kernel 2 r, stride r
        j *= int(r)
        back += int(depth) * (k - 1) * j
    return back + (k - 1) * j                                   # head


def speaking_rate(spans, max_pause: int = 6) -> Tuple[float, float]:
    """(tokens per second, seconds of speech) of one aligned row: spans (tokens, 2) = (first, last) recogniser frame per token
    (smtts_ctc_align, smtts_ctc_align_long), (-1, -1) off the path.  Over the aligned tokens in order: speech runs from the first
    token's first frame to the last token's last frame, and every gap between consecutive tokens longer than max_pause frames (6 =
    200 ms) counts as max_pause.  Frames are CTC_HOP = 800 samples at 24 kHz.  Fewer than two aligned tokens: (nan, 0.0)."""
    sp = np.asarray(spans, np.int64)
    if sp.ndim != 2 or sp.shape[1] != 2:
        raise ValueError(f"speaking_rate: spans must be (tokens, 2), got {sp.shape}")
    max_pause = int(max_pause)
    if max_pause < 0:
        raise ValueError(f"speaking_rate: max_pause must be >= 0, got {max_pause}")
    sp = sp[(sp[:, 0] >= 0) & (sp[:, 1] >= sp[:, 0])]
    if sp.shape[0] < 2:
        return float("nan"), 0.0
    gaps = sp[1:, 0] - sp[:-1, 1] - 1
    frames = int(sp[-1, 1] - sp[0, 0] + 1 - np.maximum(gaps - max_pause, 0).sum())
    seconds = frames * CTC_HOP / SAMPLE_RATE
    return sp.shape[0] / seconds, seconds


def codec_spans(spans) -> np.ndarray:
    """Token spans in recogniser frames (smtts_ctc_align) -> the codec frames they touch: (first // 4, last // 4) per token, (-1, -1)
    kept.  The result is what frames_of_groups, respeak and a Piece's `spans` count in."""
    sp = np.asarray(spans, np.int32)
    if sp.ndim != 2 or sp.shape[1] != 2:
        raise ValueError(f"codec_spans: spans must be (tokens, 2), got {sp.shape}")
    return np.where(sp < 0, np.int32(-1), sp // np.int32(CTC_FRAMES_PER_CODEC_FRAME)).astype(np.int32)


def group_confidence(groups: Sequence[Tuple[str, str, int, int]], spans, tok_logp, token0: int = 0) -> List[float]:
    """Per token group the mean over its tokens of tok_logp / span length (smtts_ctc_align's outputs of the row; span length = last -
    first + 1 frames), float32 arithmetic in token order: the mean log-probability per frame the best path gives the group, <= 0 for
    log-probabilities.  A group with a token off the path (a row that is not aligned) gets -inf."""
    out = []
    for _kind, _ph, t0, t1 in groups:
        acc, ok = np.float32(0.0), t1 > t0
        for t in range(token0 + t0, token0 + t1):
            first, last = int(spans[t][0]), int(spans[t][1])
            if first < 0 or last < first:
                ok = False
                break
            acc = np.float32(acc + np.float32(tok_logp[t]) / np.float32(last - first + 1))
        out.append(float(np.float32(acc / np.float32(t1 - t0))) if ok else float("-inf"))
    return out


def splice_pins(latents, f0: int, f1: int, m: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The pins of a re-spoken row: frames [f0, f1) of `latents` (n, 64) are replaced by m free frames (default f1 - f0, at least
    1).  -> (x_pin (n', 64) fp32, keep (n',) bool), n' = n - (f1 - f0) + m: the head [0, f0) and the tail [f1, n) are copied and
    kept (the tail at its shifted place), the m rows between them are zeros and free."""
    lat = np.asarray(latents, np.float32)
    if lat.ndim != 2 or lat.shape[1] != 64:
        raise ValueError(f"splice_pins: latents must be (n, 64), got {lat.shape}")
    n, f0, f1 = int(lat.shape[0]), int(f0), int(f1)
    if not 0 <= f0 < f1 <= n:
        raise ValueError(f"splice_pins: frames [{f0}, {f1}) must be a non-empty range inside [0, {n})")
    m = f1 - f0 if m is None else int(m)
    if m < 1:
        raise ValueError("splice_pins: at least one frame is regenerated (m >= 1)")
    x_pin = np.zeros((n - (f1 - f0) + m, 64), np.float32)
    keep = np.ones((x_pin.shape[0],), bool)
    x_pin[:f0] = lat[:f0]
    x_pin[f0 + m:] = lat[f1:]
    keep[f0:f0 + m] = False
    return x_pin, keep


def _check_pins(pins, ns: Sequence[int], start_step: int, num_steps: int):
    """synthesize_batch's pins= / start_step= -> [None | (latents (n_b, 64) fp32, keep (n_b,) bool)] per row, or None (off)."""
    start_step = int(start_step)
    if pins is None and start_step == 0:
        return None
    if not 0 <= start_step < int(num_steps):
        raise ValueError(f"synthesize_batch: start_step must lie in [0, {int(num_steps)}), got {start_step}")
    if pins is None or len(pins) != len(ns):
        raise ValueError(f"synthesize_batch: pins needs one entry per row ({len(ns)}): None or (latents, keep)"
                         + (" — start_step > 0 starts from them" if pins is None else ""))
    out = []
    for b, pe in enumerate(pins):
        if pe is None:
            if start_step > 0:
                raise ValueError(f"synthesize_batch: start_step > 0 needs latents in every row (row {b} has none)")
            out.append(None)
            continue
        if not isinstance(pe, (tuple, list)) or len(pe) != 2:
            raise ValueError(f"synthesize_batch: pins[{b}] must be None or (latents, keep)")
        lat, keep = np.asarray(pe[0]), np.asarray(pe[1])
        if lat.shape != (ns[b], 64) or lat.dtype != np.float32:
            raise ValueError(f"synthesize_batch: pins[{b}] latents must be fp32 ({ns[b]}, 64), got {lat.dtype} {lat.shape}")
        if keep.shape != (ns[b],) or keep.dtype != np.bool_:
            raise ValueError(f"synthesize_batch: pins[{b}] keep must be bool ({ns[b]},), got {keep.dtype} {keep.shape}")
        out.append((lat, keep))
    return out


def piece_seed(seed: int, i: int) -> int:
    """Seed of piece i of a long text: SeedSequence([seed, i]) reduced to 63 bits (like the replica seeds of SmallTTS)."""
    return int(np.random.SeedSequence([int(seed), int(i)]).generate_state(1, np.uint64)[0] >> 1)


def take_seed(seed: int, k: int) -> int:
    """Seed of take k of a row spoken from `seed`: take 0 is the row itself (take_seed(s, 0) == s), take k >= 1 draws from
    SeedSequence([seed, k, 0x54414B45]) reduced to 63 bits (three words: never a piece_seed)."""
    if int(k) == 0:
        return int(seed)
    return int(np.random.SeedSequence([int(seed), int(k), 0x54414B45]).generate_state(1, np.uint64)[0] >> 1)


def repair_seed(seed: int, r: int) -> int:
    """Seed of repair round r >= 1 of a row spoken from `seed`: SeedSequence([seed, r, 0x52455052]) reduced to 63 bits (three words
    with a tag of its own: never a piece_seed or a take_seed)."""
    if int(r) < 1:
        raise ValueError(f"repair_seed: rounds count from 1, got {int(r)}")
    return int(np.random.SeedSequence([int(seed), int(r), 0x52455052]).generate_state(1, np.uint64)[0] >> 1)


# ---- retiming (include/smalltts_hip.h smtts_retime): the anchor tables and the integer maps --------------------------
RETIME_MIN_SLOPE, RETIME_MAX_SLOPE = 0.125, 8.0   # what engine.retime accepts between two anchors, source samples per output sample


def retime_window(hop: int) -> np.ndarray:
    """The cross-fade window of smtts_retime, (2 hop,) fp32: w[i] = 0.5 - 0.5 cos(2 pi (i + 0.5) / (2 hop)) in float64, rounded to
    fp32 once.  w[i] rises over i < hop (the new place's weight), w[hop + i] falls (the continuation's); w[i] + w[hop + i] = 1 up to
    rounding."""
    hop = int(hop)
    if hop < 1:
        raise ValueError(f"retime_window: hop must be at least 1, got {hop}")
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(2 * hop, dtype=np.float64) + 0.5) / (2 * hop))).astype(np.float32)


def _retime_table(what: str, anchors) -> np.ndarray:
    a = np.asarray(anchors, np.int64)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 2:
        raise ValueError(f"{what}: anchors must be (m, 2) = (src, dst) with m >= 2, got {a.shape}")
    if a[0, 1] != 0 or (np.diff(a[:, 0]) <= 0).any() or (np.diff(a[:, 1]) <= 0).any() or a[0, 0] < 0:
        raise ValueError(f"{what}: the first anchor must have dst 0, and src and dst must both increase strictly")
    return a


def _retime_piecewise(what: str, v, anchors, col: int, n=None):
    """x -> y along the anchors, x read in column `col`: y_j + ((x - x_j) * (y_{j+1} - y_j)) // (x_{j+1} - x_j).  A Python int goes
    through Python's integers, an array through int64: the products stay below 2^62 for positions below 2^31."""
    a = _retime_table(what, anchors)
    xs, ys = a[:, col], a[:, 1 - col]
    if isinstance(v, (int, np.integer)):
        v = int(v)
        j = min(max(int(np.searchsorted(xs, v, side="right")) - 1, 0), len(xs) - 1)
        if j == len(xs) - 1:
            r = int(ys[j]) + (v - int(xs[j]))
        else:
            r = int(ys[j]) + ((v - int(xs[j])) * int(ys[j + 1] - ys[j])) // int(xs[j + 1] - xs[j])
        return r if n is None else min(max(r, 0), int(n))
    v = np.asarray(v, np.int64)
    j = np.clip(np.searchsorted(xs, v, side="right") - 1, 0, len(xs) - 1)
    j1 = np.minimum(j + 1, len(xs) - 1)
    den = np.where(j1 > j, xs[j1] - xs[j], 1)
    r = np.where(j1 > j, ys[j] + ((v - xs[j]) * (ys[j1] - ys[j])) // den, ys[j] + (v - xs[j]))
    return r if n is None else np.clip(r, 0, int(n))


def retime_src(t, anchors, n=None):
    """The map M of smtts_retime for a valid table (dst from 0, src and dst strictly increasing): output position t -> source
    position, s_j + ((t - d_j) * (s_{j+1} - s_j)) // (d_{j+1} - d_j) inside a pair, s_{m-1} + (t - d_{m-1}) behind the last anchor;
    with `n` clamped into [0, n].  t: a Python int or an integer array (int64 arithmetic)."""
    return _retime_piecewise("retime_src", t, anchors, 1, n)


def retime_times(s, anchors):
    """Where a source position lands: the forward map d_j + ((s - s_j) * (d_{j+1} - d_j)) // (s_{j+1} - s_j) for s_j <= s < s_{j+1},
    clamped into [d_0, d_{m-1}] outside the anchors.  Monotone; anchors map onto anchors exactly; retime_times(retime_src(t)) <= t."""
    a = _retime_table("retime_times", anchors)
    r = _retime_piecewise("retime_times", s, a, 0)
    lo, hi = int(a[0, 1]), int(a[-1, 1])
    return min(max(r, lo), hi) if isinstance(r, int) else np.clip(r, lo, hi)


def _word_span(w) -> Tuple[int, int]:
    """(start, end) of a word row: align_words' (index, kind, phonemes, start, end, confidence) or synthesize_long's (index, kind,
    start, end)."""
    return (int(w[3]), int(w[4])) if len(w) >= 6 else (int(w[2]), int(w[3]))


def _retime_words(what: str, words) -> List[Tuple[int, int, int]]:
    out = [(int(w[0]),) + _word_span(w) for w in words if w[1] == "word"]
    if any(e < s or s < 0 for _i, s, e in out) or any(b[1] < a[2] for a, b in zip(out, out[1:])):
        raise ValueError(f"{what}: the words must be in order, each with 0 <= start <= end and no overlap")
    return out


def retime_anchors(n: int, *, speed: Optional[float] = None, duration: Optional[float] = None, words=None, to_words=None,
                   min_rate: float = 0.5, max_rate: float = 2.0) -> Tuple[np.ndarray, List[int]]:
    """The anchor table of a retiming of n source samples -> (anchors (m, 2) int64 = (src, dst), the group indices of the words that
    were clamped).  Exactly one target.  `speed`: two anchors, (0, 0) and (n, round(n / speed)); `duration` seconds: (0, 0) and
    (n, round(duration * 24000)).  `to_words` (with `words`, where the words are now): both lists as align_words returns them (or
    synthesize_long's four-column rows), matched by group index over the groups of kind "word", equal counts required; anchors sit
    at every word's start and end, (0, 0) in front, the end of the audio behind at the last pause's own speed 1.  A rate is source
    samples per output sample.  A word whose rate would leave [min_rate, max_rate] keeps its start and has its length clamped, a
    pause whose rate would leave engine.retime's [1/8, 8] has its end moved to the nearest place that does.  Anchors that would not
    increase are dropped: a word that starts where the anchor in front already sits (at sample 0, or right behind the previous
    word) starts where that anchor lies, and keeps its target length from there.  Reported is every word whose start or end does
    not land on its target by retime_times, for whichever of these reasons: every word NOT reported lands exactly."""
    n = int(n)
    if n < 1:
        raise ValueError(f"retime_anchors: n must be at least 1, got {n}")
    if (speed is not None) + (duration is not None) + (to_words is not None) != 1:
        raise ValueError("retime_anchors: exactly one of speed, duration and to_words")
    if to_words is None:
        if words is not None:
            raise ValueError("retime_anchors: words belongs to to_words")
        v = float(speed if speed is not None else duration)
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError(f"retime_anchors: {'speed' if speed is not None else 'duration'} must be a positive number, got {v}")
        d = int(round(n / v)) if speed is not None else int(round(v * SAMPLE_RATE))
        if d < 1:
            raise ValueError("retime_anchors: the target is shorter than one sample")
        return np.asarray([[0, 0], [n, d]], np.int64), []
    if words is None:
        raise ValueError("retime_anchors: to_words needs words, where the words are now")
    if not (0.0 < float(min_rate) <= float(max_rate)):
        raise ValueError(f"retime_anchors: 0 < min_rate <= max_rate wanted, got {min_rate}, {max_rate}")
    lo_w, hi_w = max(float(min_rate), RETIME_MIN_SLOPE), min(float(max_rate), RETIME_MAX_SLOPE)
    src, dst = _retime_words("retime_anchors", words), _retime_words("retime_anchors", to_words)
    if len(src) != len(dst) or [w[0] for w in src] != [w[0] for w in dst]:
        raise ValueError(f"retime_anchors: words and to_words must hold the same word groups, got {len(src)} and {len(dst)}")
    if src and src[-1][2] > n:
        raise ValueError(f"retime_anchors: a word ends at {src[-1][2]}, behind the {n} samples of audio")
    rows = [(0, 0)]

    def put(s: int, d: int, lo: float, hi: float) -> None:
        s0, d0 = rows[-1]
        if s <= s0:                                             # the anchor would not increase: dropped
            return
        ds = s - s0
        d_lo, d_hi = d0 + max(1, int(np.ceil(ds / hi))), d0 + max(1, int(np.floor(ds / lo)))   # the dst that keep the rate in [lo, hi]
        rows.append((s, min(max(d, d_lo), d_hi)))

    for (_gi, s, e), (_gj, ts, te) in zip(src, dst):
        put(s, ts, RETIME_MIN_SLOPE, RETIME_MAX_SLOPE)          # the pause in front of the word
        start_d = rows[-1][1]                                   # (rows[-1][0] == s: the words are in order and do not overlap)
        put(e, start_d + (te - ts), lo_w, hi_w)                 # the word: its target length from where it starts
    if n > rows[-1][0]:
        rows.append((n, rows[-1][1] + (n - rows[-1][0])))
    if len(rows) < 2:
        raise ValueError("retime_anchors: no word to place")
    table = np.asarray(rows, np.int64)
    clamped = [gi for (gi, s, e), (_gj, ts, te) in zip(src, dst)
               if (retime_times(s, table), retime_times(e, table)) != (ts, te)]
    return table, clamped


def retime_rows(n: int, anchors, words=None, max_row: int = 30 * SAMPLE_RATE, min_pause: int = 4800):
    """Cuts a retiming of a long recording into rows that engine.retime takes side by side -> (rows, table).  `table` is `anchors`
    with every cut inserted as an anchor; it is THE map of the cut retiming (a cut inside a pair re-rounds the pair's two halves),
    and it agrees with `anchors` at every anchor.  rows = [(src offset, src length, dst offset, row anchors), ...]: each row's own
    table starts at (0, 0) and ends at (src length, dst length); source and output length of a row are both at most max_row.  Rows
    are independent chains; the result is their concatenation.  A cut lies in the middle of the last aligned pause of at least
    min_pause samples (200 ms; between consecutive groups of `words`, any kind) that keeps the row within max_row; where there is
    none, at the last anchor that does; where there is none either, at the furthest sample that does.
    A cut inside a pair gets the dst retime_times gives it, moved into the range in which BOTH halves of the pair keep a rate within
    engine.retime's [1/8, 8] and increase strictly; where rounding leaves no such dst (a pair at rate 8 cut at a source length that
    is no multiple of 8), the cut itself moves by up to 8 samples, else to the pair's nearer end.  So a table whose pairs keep the
    engine's limits is cut into rows that keep them."""
    a = _retime_table("retime_rows", anchors)
    n, max_row, min_pause = int(n), int(max_row), int(min_pause)
    if max_row < 2 or min_pause < 0:
        raise ValueError(f"retime_rows: max_row >= 2 and min_pause >= 0 wanted, got {max_row}, {min_pause}")
    end_s, end_d = int(a[-1, 0]), int(a[-1, 1])
    spans = sorted(_word_span(w) for w in (words or []))
    pauses = [(e0 + s1) // 2 for (_s0, e0), (s1, _e1) in zip(spans, spans[1:]) if s1 - e0 >= min_pause]
    table = [tuple(int(v) for v in r) for r in a]              # grows by the cuts: a later cut sees the earlier ones

    def place(c: int) -> Optional[Tuple[int, int]]:
        """A cut wanted at source sample c -> (cut, dst) on the table as it stands, or None outside it."""
        if not table[0][0] <= c <= table[-1][0]:
            return None
        j = max(i for i, r in enumerate(table) if r[0] <= c)
        if table[j][0] == c:
            return table[j]
        (sa, da), (sb, db) = table[j], table[j + 1]
        for k in sorted(range(-8, 9), key=abs):
            cc = c + k
            if not sa < cc < sb:
                continue
            lo = max(da + -(-(cc - sa) // 8), db - 8 * (sb - cc))     # both halves: ds <= 8 dd and dd <= 8 ds, dd >= 1
            hi = min(da + 8 * (cc - sa), db - -(-(sb - cc) // 8))
            if lo <= hi:
                return cc, min(max(int(retime_times(cc, np.asarray(table, np.int64))), lo), hi)
        return table[j + 1] if sb - c <= c - sa else table[j]

    def fits(s0: int, d0: int, cut: Optional[Tuple[int, int]]) -> bool:
        return cut is not None and s0 < cut[0] <= s0 + max_row and 0 < cut[1] - d0 <= max_row

    cuts, s0, d0 = [], 0, 0
    while end_s - s0 > max_row or end_d - d0 > max_row:
        cand = [cut for cut in map(place, pauses) if fits(s0, d0, cut)] or [r for r in table if fits(s0, d0, r)]
        if not cand:                                            # no pause, no anchor: the furthest sample that keeps both lengths
            now = np.asarray(table, np.int64)
            lo, hi = s0 + 1, min(s0 + max_row, end_s - 1)
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if retime_times(mid, now) - d0 <= max_row else (lo, mid - 1)
            cand = [cut for cut in (place(c) for c in range(lo, max(lo - 17, s0), -1)) if fits(s0, d0, cut)][:1]
            if not cand:
                raise ValueError("retime_rows: max_row is too small for this table")
        cut = cand[-1]
        if cut not in table:
            table = sorted(table + [cut])
        cuts.append(cut[0])
        s0, d0 = cut
    table = np.asarray(table, np.int64)
    rows, bounds = [], [0] + cuts + [end_s]
    for c0, c1 in zip(bounds, bounds[1:]):
        part = table[(table[:, 0] >= c0) & (table[:, 0] <= c1)]
        rows.append((c0, c1 - c0, int(part[0, 1]), part - part[0]))
    return rows, table


# ---- pitch (include/smalltts_hip.h smtts_pitch): the tables, f0 from the lags, per-word statistics, rows ---------------
PITCH_MAX_ROW, PITCH_CONTEXT = 30 * SAMPLE_RATE, SAMPLE_RATE   # samples of a row of SmallTTS.pitch, and what neighbours share


def pitch_tables(lmin: int, lmax: int, tilt: float = 0.1) -> np.ndarray:
    """The table of smtts_pitch, (2, L) fp32 with L = lmax - lmin + 1: row 0 lg = float32(log2(l)), row 1 tilt_l = float32(1 - tilt *
    (l - lmin) / (lmax - lmin)), both computed in float64 and rounded once.  The tilt makes a short lag win over its multiples, which
    score as high on a periodic signal."""
    lmin, lmax, tilt = int(lmin), int(lmax), float(tilt)
    if lmin < 1 or lmax <= lmin or not 0.0 <= tilt < 1.0:
        raise ValueError(f"pitch_tables: 1 <= lmin < lmax and 0 <= tilt < 1 wanted, got {lmin}, {lmax}, {tilt}")
    l = np.arange(lmin, lmax + 1, dtype=np.float64)
    return np.stack([np.log2(l), 1.0 - tilt * (l - lmin) / (lmax - lmin)]).astype(np.float32)


def pitch_f0(lag, peak, sr: float = SAMPLE_RATE) -> Tuple[np.ndarray, np.ndarray]:
    """smtts_pitch's lag (..., ) and peak (..., 3) -> (f0 in Hz, strength), float64 and float32 arrays of lag's shape.  f0 = sr /
    (l + d): d is the vertex of the parabola through the triple (S[l-1], S[l], S[l+1]), 0.5 (a - c) / (a - 2 b + c), clamped to
    [-0.5, 0.5], and 0 where the triple is flat or its middle is no maximum.  f0 is 0 where the frame is unvoiced (lag 0).  The
    strength is the score at the lag, peak[..., 1]."""
    lag = np.asarray(lag)
    pk = np.asarray(peak, np.float32)
    if pk.shape != lag.shape + (3,):
        raise ValueError(f"pitch_f0: peak must be lag's shape + (3,), got {pk.shape} for {lag.shape}")
    a, b, c = (pk[..., i].astype(np.float64) for i in range(3))
    curv = a - 2.0 * b + c
    ok = (curv < 0.0) & (b >= a) & (b >= c)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(ok, 0.5 * (a - c) / np.where(ok, curv, 1.0), 0.0)
    d = np.clip(np.where(np.isfinite(d), d, 0.0), -0.5, 0.5)
    voiced = lag > 0
    f0 = np.where(voiced, float(sr) / np.where(voiced, lag.astype(np.float64) + d, 1.0), 0.0)
    return f0, pk[..., 1].copy()


def pitch_word_stats(words, f0, hop: int) -> List[Dict[str, Optional[float]]]:
    """Per row of `words` (align_words' six columns or synthesize_long's four) one dict(f0_median, f0_min, f0_max, voiced): the median,
    the smallest and the largest f0 over the voiced frames (f0 > 0) whose start f * hop lies in [start, end), and the share of those
    frames that is voiced.  The three f0 values are None where no such frame is voiced; voiced is 0.0 where the span holds no frame."""
    f0, hop = np.asarray(f0, np.float64).reshape(-1), int(hop)
    if hop < 1:
        raise ValueError(f"pitch_word_stats: hop must be at least 1, got {hop}")
    out = []
    for w in words:
        s, e = _word_span(w)
        lo, hi = min(max(-(-s // hop), 0), f0.size), min(max(-(-e // hop), 0), f0.size)
        seg = f0[lo:hi] if hi > lo else f0[:0]
        v = seg[seg > 0.0]
        if v.size:
            out.append(dict(f0_median=float(np.median(v)), f0_min=float(v.min()), f0_max=float(v.max()), voiced=float(v.size / seg.size)))
        else:
            out.append(dict(f0_median=None, f0_min=None, f0_max=None, voiced=0.0))
    return out


def pitch_rows(n: int, hop: int, max_row: int = PITCH_MAX_ROW, context: int = PITCH_CONTEXT) -> List[Tuple[int, int, int, int]]:
    """Cuts n samples into the rows SmallTTS.pitch tracks side by side -> [(first sample, samples, first frame kept, frames kept), ...],
    frames counted over the whole signal at `hop` (frame f starts at f * hop; there are ceil(n / hop)).  Up to max_row samples: one
    row.  Longer: rows of R = max_row // hop frames (the last one shorter) whose neighbours share O = context // hop frames (made
    even), so every cut lies on a multiple of hop and a row's frames ARE the signal's frames.  Every frame is kept from the row in which
    it lies further from a cut: the shared frames are split in the middle.  Every frame is kept exactly once, in order."""
    n, hop, max_row, context = int(n), int(hop), int(max_row), int(context)
    if n < 1 or hop < 1:
        raise ValueError(f"pitch_rows: n >= 1 and hop >= 1 wanted, got {n}, {hop}")
    F, R, O = -(-n // hop), max_row // hop, (context // hop) // 2 * 2
    if R < 4 or not 2 <= O <= R // 2:
        raise ValueError(f"pitch_rows: max_row {max_row} and context {context} do not make rows at hop {hop}")
    if F <= R:
        return [(0, n, 0, F)]
    starts = [0]
    while starts[-1] + R < F:
        starts.append(starts[-1] + R - O)
    own = [0] + [s + O // 2 for s in starts[1:]] + [F]
    return [(s * hop, min(R * hop, n - s * hop), own[k], own[k + 1] - own[k]) for k, s in enumerate(starts)]
