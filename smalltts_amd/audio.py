"""Host-side audio helpers for the CLI surface: WAV read/write (PCM_16 out, like the reference's
`sf.write(..., 24000, subtype="PCM_16")`, tryme.py:29) and the Kaiser-windowed sinc resampler the
clone path uses (reference infer/utils.py:7-23: torchaudio Resample, sinc_interp_kaiser,
lowpass_filter_width=1024, rolloff=0.94, beta=14.769656459379492).  torchaudio/soundfile are not
installed here, so both are restated from their published algorithms (resampler parity unpinned)."""
from __future__ import annotations

import math
import struct
from typing import Tuple

import numpy as np

RESAMPLE_WIDTH = 1024
RESAMPLE_ROLLOFF = 0.94
RESAMPLE_BETA = 14.769656459379492

# ---- delivery: the way out of the engine (include/smalltts_hip.h smtts_deliver) ---------------------------------------
NATIVE_RATE = 24_000
DELIVER_RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
DELIVER_ENCODINGS = ("f32", "pcm16", "mulaw", "alaw")          # index = the kernel's `enc`
DELIVER_DTYPES = {"f32": np.float32, "pcm16": np.int16, "mulaw": np.uint8, "alaw": np.uint8}
# Zero crossings a side of the OUTPUT banks: 64 instead of the input side's 1024 makes the look-ahead at 8 kHz 205 samples (8.6 ms)
# instead of 3269 (136 ms), which is what a streamed consumer waits for.  A design choice, not a measurement.
DELIVER_ZEROS = 64
WAV_TAGS = {"pcm16": 1, "f32": 3, "alaw": 6, "mulaw": 7}


def deliver_ratio(rate: int) -> Tuple[int, int]:
    """-> (up, down) of NATIVE_RATE -> rate, in lowest terms; (1, 1) is the pass-through."""
    if int(rate) not in DELIVER_RATES:
        raise ValueError(f"rate must be one of {DELIVER_RATES}, got {rate!r}")
    g = math.gcd(NATIVE_RATE, int(rate))
    return int(rate) // g, NATIVE_RATE // g


def deliver_counts(n_before, length, last, up: int, down: int, width: int):
    """The integer mirror of smtts_deliver's emission rule: samples a row writes.  F(m) = max(0, (m - width) // down) frames have all
    their inputs in x[0 .. m); last == False: up * (F(n) - F(n_before)); last == True: ceil(up * n / down) - up * F(n_before), with
    n = n_before + length.  Scalars or equal-length sequences (then a list comes back)."""
    if isinstance(n_before, (list, tuple, np.ndarray)):
        ls = last if isinstance(last, (list, tuple, np.ndarray)) else [last] * len(n_before)
        return [deliver_counts(a, b, c, up, down, width) for a, b, c in zip(n_before, length, ls)]
    nb, ln = int(n_before), int(length)
    if nb < 0 or ln < 0 or up < 1 or down < 1 or width < 0:
        raise ValueError("deliver_counts: negative argument")
    F = lambda m: max(0, (m - width) // down)
    n = nb + ln
    return (-(-up * n // down) if last else up * F(n)) - up * F(nb)


def deliver_max_count(row_stride: int, up: int, down: int, width: int, streamed: bool) -> int:
    """The largest count a chunk of row_stride samples can produce (what smtts_deliver wants out_stride to hold)."""
    span = int(row_stride) + (width + down - 1 if streamed and (up, down) != (1, 1) else 0)
    return -(-up * span // down)


def _wav_header(n_bytes: int, n_samples: int, sample_rate: int, encoding: str) -> bytes:
    tag = WAV_TAGS[encoding]
    bits = {"pcm16": 16, "f32": 32, "mulaw": 8, "alaw": 8}[encoding]
    blk = bits // 8
    pad = n_bytes & 1
    if tag == 1:
        return (b"RIFF" + struct.pack("<I", 36 + n_bytes) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, 1, sample_rate, sample_rate * blk, blk, bits)
                + b"data" + struct.pack("<I", n_bytes))
    # non-PCM formats: an 18-byte fmt chunk (cbSize = 0) and a fact chunk with the sample count
    fmt = b"fmt " + struct.pack("<IHHIIHHH", 18, tag, 1, sample_rate, sample_rate * blk, blk, bits, 0)
    fact = b"fact" + struct.pack("<II", 4, n_samples)
    return b"RIFF" + struct.pack("<I", 4 + len(fmt) + len(fact) + 8 + n_bytes + pad) + b"WAVE" + fmt + fact + b"data" + struct.pack("<I", n_bytes)


def wav_bytes(samples: np.ndarray, sample_rate: int, encoding: str) -> bytes:
    """A mono WAV of ALREADY ENCODED samples, as engine.deliver returns them: int16 ("pcm16", format tag 1), uint8 G.711 codes
    ("mulaw" tag 7, "alaw" tag 6; 8 bits, with a fact chunk) or float32 ("f32", tag 3).  Nothing is converted."""
    if encoding not in WAV_TAGS:
        raise ValueError(f"encoding must be one of {DELIVER_ENCODINGS}, got {encoding!r}")
    a = np.asarray(samples).reshape(-1)
    want = DELIVER_DTYPES[encoding]
    if a.dtype != want:
        raise ValueError(f"wav_bytes: {encoding} samples must be {np.dtype(want).name}, got {a.dtype}")
    data = a.astype(a.dtype.newbyteorder("<")).tobytes()
    return _wav_header(len(data), a.size, int(sample_rate), encoding) + data + (b"\0" if len(data) & 1 else b"")


def write_wav(path: str, samples: np.ndarray, sample_rate: int, encoding: str = "pcm16") -> None:
    """wav_bytes to a file (write_wav_pcm16 stays the float -> PCM_16 writer of the CLIs)."""
    with open(path, "wb") as f:
        f.write(wav_bytes(samples, sample_rate, encoding))


class WavStreamWriter:
    """write_wav for samples that arrive in chunks (api.SmallTTS.synthesize_long_stream): the header goes out first with zero
    sizes, every write() appends ALREADY ENCODED samples, and close() pads to an even length and patches the RIFF and data sizes
    and, for G.711 and f32, the fact chunk's sample count.  The closed file equals wav_bytes of the concatenation byte for byte.
    The file must be seekable.  Also a context manager."""

    def __init__(self, path: str, sample_rate: int, encoding: str = "pcm16") -> None:
        if encoding not in WAV_TAGS:
            raise ValueError(f"encoding must be one of {DELIVER_ENCODINGS}, got {encoding!r}")
        self.sample_rate, self.encoding = int(sample_rate), encoding
        self.n_samples = self.n_bytes = 0
        self._f = open(path, "wb")
        self._f.write(_wav_header(0, 0, self.sample_rate, encoding))

    def write(self, samples: np.ndarray) -> None:
        a = np.asarray(samples).reshape(-1)
        want = DELIVER_DTYPES[self.encoding]
        if a.dtype != want:
            raise ValueError(f"WavStreamWriter: {self.encoding} samples must be {np.dtype(want).name}, got {a.dtype}")
        data = a.astype(a.dtype.newbyteorder("<")).tobytes()
        self._f.write(data)
        self.n_samples += a.size
        self.n_bytes += len(data)

    def close(self) -> None:
        if self._f is None:
            return
        if self.n_bytes & 1:
            self._f.write(b"\0")
        self._f.seek(0)
        self._f.write(_wav_header(self.n_bytes, self.n_samples, self.sample_rate, self.encoding))
        self._f.close()
        self._f = None

    def __enter__(self) -> "WavStreamWriter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()


def g711_decode(codes: np.ndarray, law: str) -> np.ndarray:
    """G.711 codes (uint8) -> int16 PCM, the CCITT / Sun g711.c decoders (audioop.ulaw2lin / alaw2lin at width 2)."""
    c = np.asarray(codes, np.uint8).astype(np.int32)
    if law == "mulaw":
        u = ~c & 0xFF
        t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
        return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)
    if law == "alaw":
        a = c ^ 0x55
        seg = (a & 0x70) >> 4
        t = (a & 0x0F) << 4
        t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
        return np.where(a & 0x80, t, -t).astype(np.int16)
    raise ValueError(f"law must be 'mulaw' or 'alaw', got {law!r}")


def write_wav_pcm16(path: str, audio: np.ndarray, sample_rate: int = 24_000) -> None:
    """float [-1,1] -> 16-bit PCM; clamp then scale by 32767 (reference server audio.rs:22-37)."""
    a = np.asarray(audio, dtype=np.float32).reshape(-1)
    pcm = np.round(np.clip(a, -1.0, 1.0) * 32767.0).astype("<i2")
    data = pcm.tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE")
        f.write(b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, sample_rate, sample_rate * 2, 2, 16))
        f.write(b"data" + struct.pack("<I", len(data)))
        f.write(data)


def read_wav(path: str) -> Tuple[np.ndarray, int]:
    """-> (float32 samples (frames,) or (frames, channels), sample_rate). PCM 8/16/24/32, float32/64 and 8-bit G.711 (tags 6, 7)."""
    with open(path, "rb") as f:
        buf = f.read()
    if buf[:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(buf):
        cid, size = buf[pos:pos + 4], struct.unpack("<I", buf[pos + 4:pos + 8])[0]
        body = buf[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
            if fmt[0] == 0xFFFE and len(body) >= 26:  # WAVE_FORMAT_EXTENSIBLE: sub-format GUID
                fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]
        elif cid == b"data":
            data = body
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f"{path}: missing fmt/data chunk")
    tag, ch, sr, _, _, bits = fmt
    if tag == 1:
        if bits == 8:
            x = (np.frombuffer(data, np.uint8).astype(np.float32) - 128.0) / 128.0
        elif bits == 16:
            x = np.frombuffer(data, "<i2").astype(np.float32) / 32768.0
        elif bits == 24:
            b = np.frombuffer(data[: len(data) // 3 * 3], np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            x = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.float32) / float(1 << 23)
        elif bits == 32:
            x = np.frombuffer(data, "<i4").astype(np.float32) / float(1 << 31)
        else:
            raise ValueError(f"{path}: unsupported PCM width {bits}")
    elif tag == 3:
        x = np.frombuffer(data, "<f4" if bits == 32 else "<f8").astype(np.float32)
    elif tag in (6, 7) and bits == 8:   # G.711 A-law / mu-law
        x = g711_decode(np.frombuffer(data, np.uint8), "alaw" if tag == 6 else "mulaw").astype(np.float32) / 32768.0
    else:
        raise ValueError(f"{path}: unsupported WAVE format tag {tag}")
    if ch > 1:
        x = x[: len(x) // ch * ch].reshape(-1, ch)
    return x, sr


def _sinc_kernel(orig: int, new: int, zeros: int = RESAMPLE_WIDTH):
    """-> (bank f32 [new][2 * width + orig], width): torchaudio's sinc_interp_kaiser bank with `zeros` zero crossings a side
    (lowpass_filter_width).  The default is the input side's bank, bit for bit what it always was."""
    base = min(orig, new) * RESAMPLE_ROLLOFF
    width = int(math.ceil(zeros * orig / base))
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base
    t = np.clip(t, -zeros, zeros)
    window = np.i0(RESAMPLE_BETA * np.sqrt(1.0 - (t / zeros) ** 2)) / np.i0(RESAMPLE_BETA)
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0.0, 1.0, np.sin(t) / t)
    return (k * window * (base / orig)).astype(np.float32), width


def resample_hq(x: np.ndarray, sr: int, target: int) -> np.ndarray:
    """(samples,) or (channels, samples) float -> resampled to `target` Hz (polyphase windowed sinc)."""
    if sr == target:
        return np.asarray(x, dtype=np.float32)
    x = np.asarray(x, dtype=np.float32)
    squeeze = x.ndim == 1
    if squeeze:
        x = x[None]
    g = math.gcd(int(sr), int(target))
    orig, new = sr // g, target // g
    kern, width = _sinc_kernel(orig, new)                      # (new, 2*width + orig)
    length = x.shape[-1]
    xp = np.pad(x, ((0, 0), (width, width + orig)))
    klen = kern.shape[1]
    n_frames = (xp.shape[-1] - klen) // orig + 1
    out = np.empty((x.shape[0], n_frames, new), dtype=np.float32)
    # strided frames (stride = orig) x polyphase bank; processed in chunks to bound memory
    win = np.lib.stride_tricks.sliding_window_view(xp, klen, axis=-1)[:, ::orig][:, :n_frames]
    step = max(1, (1 << 24) // klen)
    for s in range(0, n_frames, step):
        out[:, s:s + step] = win[:, s:s + step] @ kern.T
    y = out.reshape(x.shape[0], -1)[:, : int(math.ceil(new * length / orig))]
    return y[0] if squeeze else y
