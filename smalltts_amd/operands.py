"""The operand checks of the engine's host side as plain functions: no engine, no ctypes, no GPU (tests/test_operands_cpu.py).

One predicate, is_operand, says "a contiguous tensor of this dtype and shape on this device"; the checks below it are the ones several
engine methods share word for word.  Each takes the method's name as `what`, raises that method's ValueError and returns what the
method goes on with.  upload() is the one way a small host table reaches the device."""
from __future__ import annotations

import numpy as np
import torch

ALIGN_MAX_FRAMES, ALIGN_MAX_TOKENS = 225, 198   # smtts_align_path: 30 s of codec frames, the phoneme window


def is_operand(t, dtype, shape, device, aligned: bool = False) -> bool:
    """t is a contiguous tensor on `device` of `dtype` (or one of a tuple of dtypes) whose shape matches `shape` (None in it: any
    extent; shape=None: any rank); aligned=True: its first byte lies on a 16-byte boundary.  Anything that is no tensor answers no."""
    if not isinstance(t, torch.Tensor):
        return False
    if t.dtype not in (dtype if isinstance(dtype, tuple) else (dtype,)) or not t.is_contiguous() or t.device != device:
        return False
    if shape is not None and (t.dim() != len(shape) or any(w is not None and int(s) != w for s, w in zip(t.shape, shape))):
        return False
    return not (aligned and t.data_ptr() % 16)


def pool_slots(what: str, dev, state, sb: int, name: str, maker: str) -> int:
    """A state pool, uint8 (n_slots, sb) -> n_slots.  name / maker: what the message calls it and the method that makes one."""
    if not is_operand(state, torch.uint8, (None, sb), dev, aligned=True) or int(state.shape[0]) < 1:
        raise ValueError(f"{what}: {name} must be a contiguous, 16-byte aligned uint8 (n_slots,{sb}) tensor on the engine's device ({maker}())")
    return int(state.shape[0])


def distinct_slots(what: str, slots, B: int, n_slots: int) -> list:
    """B distinct slot indices in [0, n_slots) -> as a list of ints."""
    sl = [int(v) for v in (slots if slots is not None else [])]
    if len(sl) != B or len(set(sl)) != B or min(sl) < 0 or max(sl) >= n_slots:
        raise ValueError(f"{what}: {B} distinct slots in [0, {n_slots}) wanted, got {sl}")
    return sl


def row_lengths(what: str, lens, B: int, row: int) -> list:
    """B sample counts in [0, row] -> as a list of ints."""
    ln = [int(v) for v in lens]
    if len(ln) != B or min(ln) < 0 or max(ln) > row:
        raise ValueError(f"{what}: {B} lengths in [0, {row}] wanted, got {ln}")
    return ln


def per_row(what: str, B: int, counts, p0=None, p1=None):
    """One frame count per row and, where p0 / p1 are given, one token range."""
    if p0 is None:
        if B < 1 or len(counts) != B:
            raise ValueError(f"{what}: one frame count per row")
    elif B < 1 or len(counts) != B or len(p0) != B or len(p1) != B:
        raise ValueError(f"{what}: one frame count and one token range per row")


def frames_tokens(what: str, N: int, P: int):
    """The N / P range of the alignment kernels."""
    if not (1 <= N <= ALIGN_MAX_FRAMES and 1 <= P <= ALIGN_MAX_TOKENS):
        raise ValueError(f"{what}: N = {N}, P = {P} outside the supported range N <= {ALIGN_MAX_FRAMES}, P <= {ALIGN_MAX_TOKENS}")


def fade_len(what: str, dev, fade) -> int:
    """The optional fade table -> F, its length: 0 for None and for an empty table, which the kernels take as no fade."""
    if fade is None or (isinstance(fade, torch.Tensor) and fade.numel() == 0):
        return 0
    if not is_operand(fade, torch.float32, None, dev):
        raise ValueError(f"{what}: fade must be a contiguous fp32 tensor on the engine's device")
    return int(fade.numel())


def seg_gain(what: str, dev, B: int, seg, gain):
    """seg int64 (B,2) and the optional gain fp32 (B), as endpoints() returns them."""
    if not is_operand(seg, torch.int64, (B, 2), dev):
        raise ValueError(f"{what}: seg must be a contiguous int64 (B,2) tensor on the engine's device")
    if gain is not None and not is_operand(gain, torch.float32, (B,), dev):
        raise ValueError(f"{what}: gain must be a contiguous fp32 (B,) tensor on the engine's device, or None")


def out_1d(what: str, dev, out):
    """The joined waveform a stitch writes into."""
    if not is_operand(out, (torch.float32, torch.int16), (None,), dev):
        raise ValueError(f"{what}: out must be a contiguous 1-D fp32 or int16 tensor on the engine's device")


def upload(rows, dtype, dev) -> torch.Tensor:
    """Small per-call host table -> device tensor of `dtype` on the current stream, through pinned staging (no synchronising copy)."""
    return torch.from_numpy(np.ascontiguousarray(rows, dtype=dtype)).pin_memory().to(dev, non_blocking=True)
