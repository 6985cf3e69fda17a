"""The pure host arithmetic of the synthesis calls (api.py): text splitting, join and stream plans, token groups and word timings,
pins, seeds.  numpy only: nothing here touches the device or imports torch."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

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
