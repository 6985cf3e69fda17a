"""The option records of the synthesis calls (api.py): what `trim=`, `align=`, `takes=`, `repair=`, `deliver=`, `watermark=` and
`retime=` turn into, the Pitch record of SmallTTS.pitch, the Piece of a long take and its file.  Host only: no torch and no engine here."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .plans import SAMPLE_RATE


class _Frozen:
    """A `__slots__` class whose __init__ stores through `_set`; every later assignment or deletion raises."""
    __slots__ = ()

    def _set(self, **values) -> None:
        for k, v in values.items():
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is immutable")

    def __delattr__(self, name):
        raise AttributeError(f"{type(self).__name__} is immutable")


class _Record(_Frozen):
    """An immutable option record: repr, equality (same class, same slot values) and hash follow `__slots__` in their order."""
    __slots__ = ()

    def __repr__(self) -> str:
        return f"{type(self).__name__}(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in self.__slots__) + ")"

    def __eq__(self, other) -> bool:
        return isinstance(other, type(self)) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self) -> int:
        return hash(tuple(getattr(self, k) for k in self.__slots__))


def _coerce(cls, name: str, wanted: str, value, *, flag: bool = False, number: bool = False, pair: bool = False):
    """An option argument `name=` -> None (off) or a `cls`: None -> None and a `cls` -> itself always; with `flag` False -> None and
    True -> cls(); with `number` an int (never a bool) -> cls(int); with `pair` a 2-tuple or 2-list -> cls(first, second).  Anything
    else: TypeError, `wanted` naming what is accepted."""
    if value is None or isinstance(value, cls):
        return value
    if isinstance(value, bool):
        if flag:
            return cls() if value else None
    elif number and isinstance(value, (int, np.integer)):
        return cls(int(value))
    elif pair and isinstance(value, (tuple, list)) and len(value) == 2:
        return cls(value[0], value[1])
    raise TypeError(f"{name} must be None, {wanted}, got {type(value).__name__}")


class Endpointing(_Record):
    """How the ends of the speech in a row are found, and how the row is levelled (immutable; DESIGN 8a, include/smalltts_hip.h
    smtts_endpoints).  frame_ms: analysis frame; a frame is active when its mean power is above both `rel_db` below the row's
    loudest frame and `floor_dbfs`; speech = runs of at least `min_run` active frames; `lead_ms` / `tail_ms` are kept in front of the
    first / behind the last speech frame.  level_dbfs None: no gain; else the speech frames' RMS is brought to it, by at most
    `max_gain_db`, and never so far that the row's peak passes `peak_dbfs`."""
    __slots__ = ("frame_ms", "rel_db", "floor_dbfs", "min_run", "lead_ms", "tail_ms", "level_dbfs", "peak_dbfs", "max_gain_db")

    def __init__(self, frame_ms: float = 10.0, rel_db: float = 40.0, floor_dbfs: float = -80.0, min_run: int = 3, lead_ms: float = 30.0,
                 tail_ms: float = 60.0, level_dbfs: Optional[float] = None, peak_dbfs: float = -1.0, max_gain_db: float = 20.0) -> None:
        self._set(frame_ms=float(frame_ms), rel_db=float(rel_db), floor_dbfs=float(floor_dbfs), min_run=int(min_run),
                  lead_ms=float(lead_ms), tail_ms=float(tail_ms), level_dbfs=None if level_dbfs is None else float(level_dbfs),
                  peak_dbfs=float(peak_dbfs), max_gain_db=float(max_gain_db))
        W = 4 * int(round(self.frame_ms * SAMPLE_RATE / 1000.0 / 4))
        if not 16 <= W <= 4096:
            raise ValueError(f"Endpointing: frame_ms = {frame_ms} gives a frame of {W} samples, outside [16, 4096]")
        if not 1 <= self.min_run <= 16:
            raise ValueError("Endpointing: min_run must be in [1, 16]")
        if self.lead_ms < 0 or self.tail_ms < 0 or self.rel_db < 0:
            raise ValueError("Endpointing: lead_ms, tail_ms and rel_db must not be negative")
        if not all(np.isfinite(v) for v in (self.frame_ms, self.rel_db, self.floor_dbfs, self.lead_ms, self.tail_ms, self.peak_dbfs,
                                            self.max_gain_db, 0.0 if self.level_dbfs is None else self.level_dbfs)):
            raise ValueError("Endpointing: every parameter must be finite")

    def kernel_params(self) -> Dict[str, object]:
        """The kernel's parameters: float64 arithmetic, rounded to fp32 once.  W = 4 round(frame_ms * 24 / 4) samples, rel_pow =
        10^(-rel_db / 10), floor_pow = 10^(floor_dbfs / 10), lead / tail = round(ms * 24) samples, target_rms = 10^(level_dbfs / 20)
        (0 = no gain), peak_limit = 10^(peak_dbfs / 20), max_gain = 10^(max_gain_db / 20)."""
        f32 = lambda v: np.float32(np.float64(v))
        per_ms = SAMPLE_RATE / 1000.0
        return {"W": 4 * int(round(self.frame_ms * per_ms / 4)), "rel_pow": f32(10.0 ** (-self.rel_db / 10.0)),
                "floor_pow": f32(10.0 ** (self.floor_dbfs / 10.0)), "min_run": self.min_run,
                "lead": int(round(self.lead_ms * per_ms)), "tail": int(round(self.tail_ms * per_ms)),
                "target_rms": np.float32(0.0) if self.level_dbfs is None else f32(10.0 ** (self.level_dbfs / 20.0)),
                "peak_limit": f32(10.0 ** (self.peak_dbfs / 20.0)), "max_gain": f32(10.0 ** (self.max_gain_db / 20.0))}


def as_endpointing(trim) -> Optional["Endpointing"]:
    """The `trim=` argument of the synthesis calls: None / False -> None (off), True -> Endpointing(), an Endpointing -> itself."""
    return _coerce(Endpointing, "trim", "a bool or an Endpointing", trim, flag=True)


class Alignment(_Record):
    """Which text-attention probabilities the word timings are read from (immutable; DESIGN 'Word timings', include/smalltts_hip.h
    smtts_sample_align).  layers: DiT blocks in [0, 12); heads: attention heads in [0, 8); steps: sampler steps, indices into
    range(num_steps), negative from the end.  None = the default of each: ALL layers, ALL heads, the LAST step (t = 0, where x_t is
    the current estimate itself).  The result is the mean over the selected (step, layer, head) triples.

    The default is UNVALIDATED on trained weights: every weight this project has run is seeded noise, and nobody has measured in
    which layers and heads this model's text attention is monotone and peaky.  The mechanism is verified (the probabilities, the
    optimal monotone path, the mapping to samples); the selection is a parameter for whoever holds a trained checkpoint.
    Resolution: one codec frame, 3200 samples = 133 ms — word highlighting and subtitles, not lip-sync."""
    __slots__ = ("layers", "heads", "steps")

    def __init__(self, layers: Optional[Sequence[int]] = None, heads: Optional[Sequence[int]] = None,
                 steps: Optional[Sequence[int]] = None) -> None:
        for k, v, n in (("layers", layers, 12), ("heads", heads, 8), ("steps", steps, None)):
            if v is not None:
                v = tuple(sorted(set(int(i) for i in v)))
                if not v:
                    raise ValueError(f"Alignment: {k} must not be empty (None = the default)")
                if n is not None and (v[0] < 0 or v[-1] >= n):
                    raise ValueError(f"Alignment: {k} must lie in [0, {n}), got {v}")
            self._set(**{k: v})


def as_alignment(align) -> Optional["Alignment"]:
    """The `align=` argument of the synthesis calls: None / False -> None (off), True -> Alignment(), an Alignment -> itself."""
    return _coerce(Alignment, "align", "a bool or an Alignment", align, flag=True)


ALIGN_MAX_FRAMES, ALIGN_MAX_TOKENS = 225, 198   # the range of smtts_align_path: 30 s of frames, the phoneme window


class Takes(_Record):
    """Best-of-K sampling (immutable; DESIGN 8d, include/smalltts_hip.h smtts_take_scores / smtts_take_select): every row is sampled
    `k` times (1..16) from seeds take_seed(seed, 0 .. k-1), each take's text alignment is scored on the device and only the take with
    the lowest total is decoded.  total = w0 * path cost per cell + w1 * skipped tokens / tokens + w2 * longest span / frames + w3 *
    idle frames / frames with `weights` = (w0, w1, w2, w3), all >= 0; a token is skipped when no frame of its span gives it
    `tau_token` of its attention, a frame is idle when it gives no token of the row `tau_frame`.

    The defaults are design choices, not measurements.  What the score is worth is UNVALIDATED on trained weights: every weight this
    project has run is seeded noise, nobody has measured whether the lowest total is the take a listener would keep, and the score
    rests on the tap's layer / head selection (Alignment), which is unvalidated in the same way.  The mechanism is verified: the
    features and the total (bit for bit against a numpy restatement), the selection, and that the winner's latents, audio and words
    are those of the same row sampled alone.

    `ctc` (>= 0, default 0 = off: the launches and bits of the score above): a CTC term.  The latent phoneme recogniser
    (engine part "asr", SmallTTS(recogniser=True)) reads every take's latents, nll = the CTC negative log-likelihood of the row's
    spoken tokens (smtts_ctc_score), and total' = total + (ctc * nll) / tokens, three single fp32 operations in that order.  It asks
    "were these phonemes spoken?" and is the quantity the 4-step student was distilled to make small; UNVALIDATED in the same way:
    no recogniser checkpoint has ever been loaded, and its Conformer composition is restated from recollection.  Not with repair=.

    `sv` (>= 0, default 0 = off: not one launch more, not one bit changed): a speaker term.  The latent speaker verifier
    (engine part "sv", SmallTTS(verifier=True)) embeds every take's latents (smtts_sv_embed), cos = the cosine of that embedding with
    the reference voice's (smtts_sv_cosine; the Voice's `speaker`, or the embedding of the row's ref_latents), and
    total' = total + sv * (1 - cos), three single fp32 operations in that order, behind the CTC term where that is on.  It asks "does
    this take sound like the reference voice?" and is the third quantity the 4-step student was distilled to make small; UNVALIDATED
    in the same way: no verifier checkpoint has ever been loaded, its ECAPA composition is restated from recollection, and the weight
    is a design choice.  Every row and every reference needs 6 to 225 frames.  Not with repair=."""
    __slots__ = ("k", "weights", "tau_token", "tau_frame", "ctc", "sv")
    MAX_K, MAX_ROWS = 16, 64   # smtts_take_select's K; the largest sampler batch the tap is tested at

    def __init__(self, k: int, weights: Sequence[float] = (1.0, 2.0, 1.0, 1.0), tau_token: float = 0.1, tau_frame: float = 0.1,
                 ctc: float = 0.0, sv: float = 0.0) -> None:
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"Takes: k must be an integer, got {type(k).__name__}")
        if not 1 <= int(k) <= self.MAX_K:
            raise ValueError(f"Takes: k must lie in [1, {self.MAX_K}], got {int(k)}")
        w = tuple(float(v) for v in weights)
        if len(w) != 4 or not all(v >= 0.0 and np.isfinite(v) for v in w):
            raise ValueError(f"Takes: weights must be four finite numbers >= 0, got {w}")
        if not (np.isfinite(float(tau_token)) and np.isfinite(float(tau_frame))):
            raise ValueError("Takes: tau_token and tau_frame must be finite")
        if isinstance(ctc, bool) or not (np.isfinite(float(ctc)) and float(ctc) >= 0.0):
            raise ValueError(f"Takes: ctc must be a finite number >= 0, got {ctc!r}")
        if isinstance(sv, bool) or not (np.isfinite(float(sv)) and float(sv) >= 0.0):
            raise ValueError(f"Takes: sv must be a finite number >= 0, got {sv!r}")
        self._set(k=int(k), weights=w, tau_token=float(tau_token), tau_frame=float(tau_frame), ctc=float(ctc), sv=float(sv))


def as_takes(takes) -> Optional["Takes"]:
    """The `takes=` argument of the synthesis calls: None -> None (off), an int K -> Takes(K), a Takes -> itself."""
    return _coerce(Takes, "takes", "an int or a Takes", takes, number=True)


class Repair(_Record):
    """Repair of a take (immutable; DESIGN 8e, include/smalltts_hip.h smtts_repair_plan / smtts_repair_keep): behind the sampler (and
    the take selection) the tokens of every row whose alignment is bad are found on the device, only their frames are drawn again by
    one pinned sampler pass with every other frame held to the row's latents, the row is scored again, and the repaired row is kept
    only where its total is strictly lower; `rounds` (1..4) such passes.  A token is bad when its span on the monotone path is empty,
    longer than `max_span` frames (1..225), or holds no frame that gives the token `tau_token` of its attention; a bad token frees its
    span plus `margin` frames (0..32) on either side.  The total is the call's Takes' (the default weights without `takes`).

    The defaults are design choices, not measurements.  Repair is UNVALIDATED on trained weights: every weight this project has run
    is seeded noise, nobody has measured whether a 4-step student inpaints the freed frames audibly well, and nobody has measured
    whether a lower total is the better take.  The mechanism is verified: the plan and the keep rule (bit for bit against a numpy
    restatement), that a repaired row is the pinned call by hand, and that every frame the plan pinned keeps its bits."""
    __slots__ = ("rounds", "tau_token", "max_span", "margin")
    MAX_ROUNDS, MAX_MARGIN = 4, 32

    def __init__(self, rounds: int = 1, tau_token: float = 0.1, max_span: int = 8, margin: int = 2) -> None:
        for name, v in (("rounds", rounds), ("max_span", max_span), ("margin", margin)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"Repair: {name} must be an integer, got {type(v).__name__}")
        if not 1 <= int(rounds) <= self.MAX_ROUNDS:
            raise ValueError(f"Repair: rounds must lie in [1, {self.MAX_ROUNDS}], got {int(rounds)}")
        if not 1 <= int(max_span) <= ALIGN_MAX_FRAMES:
            raise ValueError(f"Repair: max_span must lie in [1, {ALIGN_MAX_FRAMES}], got {int(max_span)}")
        if not 0 <= int(margin) <= self.MAX_MARGIN:
            raise ValueError(f"Repair: margin must lie in [0, {self.MAX_MARGIN}], got {int(margin)}")
        if not np.isfinite(float(tau_token)):
            raise ValueError("Repair: tau_token must be finite")
        self._set(rounds=int(rounds), tau_token=float(tau_token), max_span=int(max_span), margin=int(margin))


def as_repair(repair) -> Optional["Repair"]:
    """The `repair=` argument of the synthesis calls: None -> None (off), an int -> Repair(rounds), a Repair -> itself."""
    return _coerce(Repair, "repair", "an int or a Repair", repair, number=True)


class Delivery(_Record):
    """The rate and encoding audio leaves the engine in (immutable; DESIGN 8g, include/smalltts_hip.h smtts_deliver): `rate` one of
    8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000 Hz, `encoding` "f32" | "pcm16" | "mulaw" | "alaw" (G.711, audioop's codes).
    Resampled and encoded on the device behind the decode, whole or in chunks that continue each other bit for bit.  The banks are
    the project's Kaiser-sinc restatement with audio.DELIVER_ZEROS zero crossings: unpinned against torchaudio, a design choice."""
    __slots__ = ("rate", "encoding")

    def __init__(self, rate: int = 24_000, encoding: str = "f32") -> None:
        from .audio import DELIVER_ENCODINGS, DELIVER_RATES
        if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)):
            raise TypeError(f"Delivery: rate must be an integer, got {type(rate).__name__}")
        if int(rate) not in DELIVER_RATES:
            raise ValueError(f"Delivery: rate must be one of {DELIVER_RATES}, got {int(rate)}")
        if encoding not in DELIVER_ENCODINGS:
            raise ValueError(f"Delivery: encoding must be one of {DELIVER_ENCODINGS}, got {encoding!r}")
        self._set(rate=int(rate), encoding=str(encoding))

    @property
    def ratio(self) -> Tuple[int, int]:
        """(up, down) of 24 kHz -> rate in lowest terms."""
        from .audio import deliver_ratio
        return deliver_ratio(self.rate)

    @property
    def dtype(self):
        from .audio import DELIVER_DTYPES
        return DELIVER_DTYPES[self.encoding]

    def samples(self, s: int) -> int:
        """A position or length of `s` samples at 24 kHz in output samples: ceil(up * s / down)."""
        up, down = self.ratio
        return -(-up * int(s) // down)


def as_delivery(deliver) -> Optional["Delivery"]:
    """The `deliver=` argument of the synthesis calls: None -> None (today's path: 24 kHz fp32, not one launch more), a Delivery ->
    itself, an int -> Delivery(rate), a (rate, encoding) pair -> Delivery(rate, encoding)."""
    return _coerce(Delivery, "deliver", "a Delivery, a rate or a (rate, encoding) pair", deliver, number=True, pair=True)


class Watermark(_Record):
    """A keyed watermark on the audio the engine hands out (immutable; DESIGN 8k, include/smalltts_hip.h smtts_watermark): `key` an
    integer in [0, 2^64), the shared secret the detector needs (whoever holds it can also strip the mark); `strength` in [0, 1], the
    mark's amplitude relative to the RMS of the 64 samples in front (0.02: 34 dB below the signal; a design choice that has never
    been listened to).  Embedded on the device at 24 kHz in front of the delivery, whole or in chunks that continue each other bit
    for bit; SmallTTS.detect_watermark finds it again in f32 or PCM16 audio, also cropped from the front.  Detection is unvalidated
    on real speech and on trained weights."""
    __slots__ = ("key", "strength")

    def __init__(self, key: int, strength: float = 0.02) -> None:
        if isinstance(key, bool) or not isinstance(key, (int, np.integer)):
            raise TypeError(f"Watermark: key must be an integer, got {type(key).__name__}")
        if not 0 <= int(key) < 2 ** 64:
            raise ValueError(f"Watermark: key must be in [0, 2^64), got {int(key)}")
        if isinstance(strength, bool) or not isinstance(strength, (int, float, np.integer, np.floating)):
            raise TypeError(f"Watermark: strength must be a number, got {type(strength).__name__}")
        if not (0.0 <= float(strength) <= 1.0):                # (also refuses NaN)
            raise ValueError(f"Watermark: strength must be in [0, 1], got {float(strength)}")
        self._set(key=int(key), strength=float(strength))


def as_watermark(watermark) -> Optional["Watermark"]:
    """The `watermark=` argument of the synthesis calls: None -> None (no mark, not one launch more), a Watermark -> itself, an
    int -> Watermark(key), a (key, strength) pair -> Watermark(key, strength)."""
    return _coerce(Watermark, "watermark", "a Watermark, a key or a (key, strength) pair", watermark, number=True, pair=True)


def marked_delivery(what: str, watermark, dv: Optional["Delivery"]):
    """watermark= next to deliver= -> (Watermark or None, Delivery or None).  A mark without deliver= leaves as Delivery(24000, "f32");
    any other rate, and G.711, are refused: the mark lives mostly above 4 kHz and is about as large as G.711's own noise, it would
    not survive, and a silent no-op is worse than a refusal."""
    wm = as_watermark(watermark)
    if wm is None:
        return None, dv
    if dv is None:
        dv = Delivery(24_000, "f32")
    if dv.rate != 24_000 or dv.encoding not in ("f32", "pcm16"):
        raise ValueError(f"{what}: watermark= needs 24000 Hz and f32 or pcm16 (the mark would not survive resampling or G.711), "
                         f"got {dv!r}")
    return wm, dv


class Retime(_Record):
    """A retiming of the 24 kHz waveform on the device (immutable; DESIGN 8n, include/smalltts_hip.h smtts_retime): WSOLA onto
    exactly one target.  `speed` > 0: the audio runs `speed` times as fast, round(n / speed) samples; `duration` > 0 seconds: it
    lasts round(duration * 24000) samples; `to_words`: word rows as align_words returns them, where every word shall lie
    (SmallTTS.retime, together with the words' present times).  `hop` (a multiple of 4 in [16, 512]) is the segment, `delta` (0 ..
    512) how far a segment's source may lie from where the map says.  `min_rate` / `max_rate` bound a word's rate (source samples
    per output sample) under to_words; a word outside keeps its start, has its length clamped and is reported.  Pitch is kept; how
    retimed speech sounds has never been listened to: only the signal properties of DESIGN 8n are tested."""
    __slots__ = ("speed", "duration", "to_words", "hop", "delta", "min_rate", "max_rate")

    def __init__(self, speed: Optional[float] = None, duration: Optional[float] = None, to_words=None, hop: int = 240, delta: int = 120,
                 min_rate: float = 0.5, max_rate: float = 2.0) -> None:
        if (speed is not None) + (duration is not None) + (to_words is not None) != 1:
            raise ValueError("Retime: exactly one of speed, duration and to_words")
        for name, v in (("speed", speed), ("duration", duration)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating))):
                raise TypeError(f"Retime: {name} must be a number, got {type(v).__name__}")
            if v is not None and not (np.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError(f"Retime: {name} must be a positive number, got {v!r}")
        for name, v in (("hop", hop), ("delta", delta)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"Retime: {name} must be an integer, got {type(v).__name__}")
        if not 16 <= int(hop) <= 512 or int(hop) % 4:
            raise ValueError(f"Retime: hop must be a multiple of 4 in [16, 512], got {int(hop)}")
        if not 0 <= int(delta) <= 512:
            raise ValueError(f"Retime: delta must lie in [0, 512], got {int(delta)}")
        if not (np.isfinite(float(min_rate)) and np.isfinite(float(max_rate)) and 0.0 < float(min_rate) <= float(max_rate)):
            raise ValueError(f"Retime: 0 < min_rate <= max_rate wanted, got {min_rate!r}, {max_rate!r}")
        if to_words is not None:
            to_words = tuple(tuple(w) for w in to_words)
            if not to_words or not all(len(w) >= 4 for w in to_words):
                raise ValueError("Retime: to_words must be a non-empty list of word rows (align_words)")
        self._set(speed=None if speed is None else float(speed), duration=None if duration is None else float(duration),
                  to_words=to_words, hop=int(hop), delta=int(delta), min_rate=float(min_rate), max_rate=float(max_rate))


def as_retime(retime) -> Optional["Retime"]:
    """The `retime=` argument: None -> None (off: the call as it always was), a Retime -> itself, a number -> Retime(speed=number)."""
    if retime is None or isinstance(retime, Retime):
        return retime
    if not isinstance(retime, bool) and isinstance(retime, (int, float, np.integer, np.floating)):
        return Retime(speed=float(retime))
    raise TypeError(f"retime must be None, a speed or a Retime, got {type(retime).__name__}")


class Pitch(_Record):
    """How SmallTTS.pitch tracks F0 on the device (immutable; DESIGN 8o, include/smalltts_hip.h smtts_pitch).  Candidates are the lags
    `lmin` = floor(24000 / fmax) .. `lmax` = ceil(24000 / fmin) samples; a frame starts every `hop` samples (a multiple of 4 in [16,
    1024]) and correlates `win` samples (a multiple of 4 in [32, 2048]); `floor_pow` is the power below which a frame counts as
    silence (the score's bias is (win * floor_pow)^2); `tilt` is how much of its score the longest lag loses against the shortest;
    `c_unv` is the cost of an unvoiced frame (a voiced one costs 1 - score * tilt_l), `w_jump` the cost per octave of a jump between
    consecutive voiced frames, `w_switch` the cost of a change of voicing.  The limits: 2 <= lmin < lmax <= 2048 and at most 1023
    lags.  The constants are design choices checked on synthetic signals only (tones, noise, silence): they are NOT tuned on speech,
    and nothing about accuracy on real speech is claimed."""
    __slots__ = ("fmin", "fmax", "hop", "win", "floor_pow", "tilt", "c_unv", "w_jump", "w_switch", "lmin", "lmax")

    def __init__(self, fmin: float = 60.0, fmax: float = 400.0, hop: int = 240, win: int = 480, floor_pow: float = 1e-6,
                 tilt: float = 0.1, c_unv: float = 0.55, w_jump: float = 0.35, w_switch: float = 0.3) -> None:
        nums = (("fmin", fmin), ("fmax", fmax), ("floor_pow", floor_pow), ("tilt", tilt), ("c_unv", c_unv), ("w_jump", w_jump),
                ("w_switch", w_switch))
        for name, v in nums:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError(f"Pitch: {name} must be a number, got {type(v).__name__}")
            if not np.isfinite(float(v)):
                raise ValueError(f"Pitch: {name} must be finite, got {v!r}")
        for name, v in (("hop", hop), ("win", win)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"Pitch: {name} must be an integer, got {type(v).__name__}")
        if not 16 <= int(hop) <= 1024 or int(hop) % 4:
            raise ValueError(f"Pitch: hop must be a multiple of 4 in [16, 1024], got {int(hop)}")
        if not 32 <= int(win) <= 2048 or int(win) % 4:
            raise ValueError(f"Pitch: win must be a multiple of 4 in [32, 2048], got {int(win)}")
        if not 0.0 < float(fmin) < float(fmax):
            raise ValueError(f"Pitch: 0 < fmin < fmax wanted, got {fmin!r}, {fmax!r}")
        lmin, lmax = int(np.floor(24000.0 / float(fmax))), int(np.ceil(24000.0 / float(fmin)))
        if lmin < 2 or lmax <= lmin or lmax > 2048 or lmax - lmin + 1 > 1023:
            raise ValueError(f"Pitch: fmin = {fmin!r}, fmax = {fmax!r} give the lags {lmin} .. {lmax}; 2 <= lmin < lmax <= 2048 and at most "
                             "1023 lags wanted")
        if not float(floor_pow) > 0.0:
            raise ValueError(f"Pitch: floor_pow must be positive, got {floor_pow!r}")
        if not 0.0 <= float(tilt) < 1.0:
            raise ValueError(f"Pitch: tilt must lie in [0, 1), got {tilt!r}")
        for name, v in (("c_unv", c_unv), ("w_jump", w_jump), ("w_switch", w_switch)):
            if float(v) < 0.0:
                raise ValueError(f"Pitch: {name} must not be negative, got {v!r}")
        self._set(fmin=float(fmin), fmax=float(fmax), hop=int(hop), win=int(win), floor_pow=float(floor_pow), tilt=float(tilt),
                  c_unv=float(c_unv), w_jump=float(w_jump), w_switch=float(w_switch), lmin=lmin, lmax=lmax)

    @property
    def bias(self) -> float:
        """What smtts_pitch adds under the root: (win * floor_pow)^2."""
        return (self.win * self.floor_pow) ** 2


def as_pitch(pitch) -> "Pitch":
    """The `pitch=` argument: None -> Pitch() (the defaults), a Pitch -> itself."""
    if pitch is None:
        return Pitch()
    if isinstance(pitch, Pitch):
        return pitch
    raise TypeError(f"pitch must be None or a Pitch, got {type(pitch).__name__}")


class Piece(_Frozen):
    """One piece of a long take, as synthesize_long(return_pieces=True) spoke it: `tokens` (the prefix included), `prefix_len` (how
    many of them are the prepended transcription), `latents` (n, 64) fp32 on the host, and the `seed` of its noise; `spans`
    (len(tokens), 2) int32, the (first, last) frame of every token, when the take was aligned (return_words, or SmallTTS.realign),
    else None.  Immutable; render_long joins pieces again, respeak makes the latents of a replacement."""
    __slots__ = ("tokens", "prefix_len", "latents", "seed", "spans")

    def __init__(self, tokens: Sequence[int], prefix_len: int, latents, seed: int, spans=None) -> None:
        lat = np.array(latents, np.float32)
        if lat.ndim != 2 or lat.shape[1] != 64 or lat.shape[0] < 1:
            raise ValueError(f"Piece: latents must be (n, 64) with n >= 1, got {lat.shape}")
        if not 0 <= int(prefix_len) <= len(tokens):
            raise ValueError("Piece: prefix_len must lie in [0, len(tokens)]")
        lat.setflags(write=False)
        self._set(tokens=tuple(int(t) for t in tokens), prefix_len=int(prefix_len), latents=lat, seed=int(seed))
        if spans is not None:
            spans = np.array(spans, np.int32)
            if spans.shape != (len(self.tokens), 2):
                raise ValueError(f"Piece: spans must be ({len(self.tokens)}, 2), one (first, last) frame per token, got {spans.shape}")
            spans.setflags(write=False)
        self._set(spans=spans)

    def __repr__(self) -> str:
        return f"Piece(tokens={len(self.tokens)}, prefix_len={self.prefix_len}, frames={self.latents.shape[0]}, seed={self.seed})"


TAKE_JOIN_KEYS = ("gap_ms", "fade_ms", "max_batch", "in_flight", "trim", "level_dbfs")


def save_take(path, pieces: Sequence["Piece"], **join) -> None:
    """A long take -> one .npz: every Piece (tokens, prefix_len, latents, seed, spans when it has them) and the join parameters
    (TAKE_JOIN_KEYS: gap_ms, fade_ms, max_batch, in_flight, trim as a bool, level_dbfs or None), enough for render_long to give the
    waveform again.  Plain arrays only (no pickle)."""
    unknown = sorted(set(join) - set(TAKE_JOIN_KEYS))
    if unknown:
        raise ValueError(f"save_take: unknown join parameters {unknown}")
    level = join.get("level_dbfs")
    arrs = {"n_pieces": np.int64(len(pieces)), "prefix_len": np.asarray([p.prefix_len for p in pieces], np.int64),
            "seed": np.asarray([p.seed for p in pieces], np.uint64), "gap_ms": np.float64(join.get("gap_ms", 120.0)),
            "fade_ms": np.float64(join.get("fade_ms", 5.0)), "max_batch": np.int64(join.get("max_batch", 8)),
            "in_flight": np.int64(join.get("in_flight", 3)), "trim": np.bool_(join.get("trim", False)),
            "level_dbfs": np.float64(np.nan if level is None else level)}
    for i, p in enumerate(pieces):
        arrs[f"tokens_{i}"] = np.asarray(p.tokens, np.int64)
        arrs[f"latents_{i}"] = np.asarray(p.latents, np.float32)
        if p.spans is not None:
            arrs[f"spans_{i}"] = np.asarray(p.spans, np.int32)
    with open(path, "wb") as f:
        np.savez(f, **arrs)


def load_take(path) -> Tuple[List["Piece"], Dict[str, object]]:
    """save_take's file -> (pieces, join parameters as keyword arguments of save_take)."""
    with np.load(path, allow_pickle=False) as z:
        n = int(z["n_pieces"])
        pieces = [Piece(z[f"tokens_{i}"].tolist(), int(z["prefix_len"][i]), z[f"latents_{i}"], int(z["seed"][i]),
                        z[f"spans_{i}"] if f"spans_{i}" in z.files else None) for i in range(n)]
        level = float(z["level_dbfs"])
        join = {"gap_ms": float(z["gap_ms"]), "fade_ms": float(z["fade_ms"]), "max_batch": int(z["max_batch"]),
                "in_flight": int(z["in_flight"]), "trim": bool(z["trim"]), "level_dbfs": None if np.isnan(level) else level}
    return pieces, join
