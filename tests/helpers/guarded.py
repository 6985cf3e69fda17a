"""A guarded allocator for the bounds tests (tests/test_bounds_gpu.py; the checker itself: tests/test_guarded_cpu.py).  Plain torch, CPU
or GPU.

Every buffer of a call (input, output, workspace) is a view into a uint8 allocation of its own:

    [ front guard >= `guard` bytes | payload, 256-byte aligned start, exactly nbytes | rear guard, `guard` bytes ]

The rear guard begins at the byte right after the payload's last byte, not at the next aligned boundary, so a write one element past
an odd-sized output lands in it.  A kernel that writes outside what it was handed changes guard bytes, which check() reports; a kernel
that reads outside and uses the value gives other results when the guards are painted 0x00 than when they are painted 0xFF (NaN as fp32,
-1 as int64, "true" as a mask byte).  Neither can fault: every byte watched belongs to the test's own allocation.

The guard width is derived, not tuned: the largest overrun a tile bug can produce in this project is one 160-row GEMM tile of a
2432-column 16-bit operand image, 160 * 2432 * 2 = 778 240 bytes (about 760 KiB) < 1 MiB."""
from collections import namedtuple

import numpy as np
import torch

GUARD = 1 << 20
ALIGN = 256


class Damage(namedtuple("Damage", "name side offset count")):
    """One damaged guard.  side "front" / "rear"; offset of the first changed byte relative to the payload's edge: rear +0 is the byte
    right behind the payload, front -1 the byte right in front of it; count = changed bytes in that guard."""

    def __str__(self):
        return f"`{self.name}` {self.side} {self.offset:+d}, {self.count} byte{'s' if self.count != 1 else ''}"


class _Buf:
    __slots__ = ("name", "raw", "start", "nbytes", "edge", "role", "view")


class Arena:
    """Arena(device, guard=1 << 20): the buffers of one call.  role "in" payloads are left as the test set them; "out" and "ws"
    payloads are zeroed by every paint(), the same in every run."""

    def __init__(self, device, guard: int = GUARD):
        self.device = torch.device(device)
        self.guard = int(guard)
        self.bufs = {}
        self.byte = None

    # ---- allocation ---------------------------------------------------------------------------------------------------------
    def alloc(self, name: str, shape, dtype, role: str = "out", skew: int = 0) -> torch.Tensor:
        """A tensor of `shape` / `dtype` between guards.  skew: bytes the payload start is moved behind its 256-byte boundary (the
        one case that needs an address that is 4-byte but not 16-byte aligned); a multiple of the element size."""
        assert name not in self.bufs and role in ("in", "out", "ws"), (name, role)
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * item
        assert 0 <= skew < ALIGN and skew % item == 0
        b = _Buf()
        b.name, b.role, b.nbytes = name, role, nbytes
        b.raw = torch.empty(self.guard + ALIGN + skew + nbytes + self.guard, dtype=torch.uint8, device=self.device)
        b.start = self.guard + (-(b.raw.data_ptr() + self.guard)) % ALIGN + skew
        b.edge = b.start + nbytes                       # where the rear guard begins
        b.view = b.raw[b.start:b.edge].view(dtype).view(shape)
        assert b.view.data_ptr() == b.raw.data_ptr() + b.start and (b.view.data_ptr() - skew) % ALIGN == 0
        self.bufs[name] = b
        return b.view

    def put(self, name: str, t: torch.Tensor, skew: int = 0) -> torch.Tensor:
        """An input: a guarded copy of `t` (any device)."""
        v = self.alloc(name, t.shape, t.dtype, role="in", skew=skew)
        v.copy_(t)
        return v

    def workspace(self, name: str, nbytes: int) -> torch.Tensor:
        """A workspace of exactly `nbytes` bytes (what the *_workspace_bytes call returned)."""
        return self.alloc(name, (int(nbytes),), torch.uint8, role="ws")

    def claim(self, name: str, nbytes: int):
        """Tells the checker that `name`'s payload ends after `nbytes` bytes: the rest of the true payload counts as rear guard from
        the next paint() on.  The bytes stay inside the allocation; the self-test of tests/test_bounds_gpu.py hands them to the
        engine in full and expects the damage report."""
        b = self.bufs[name]
        assert 0 <= nbytes <= b.nbytes
        b.edge = b.start + int(nbytes)

    def __getitem__(self, name: str) -> torch.Tensor:
        return self.bufs[name].view

    # ---- painting -------------------------------------------------------------------------------------------------------------
    def _guards(self, b):
        return (("front", b.raw[:b.start]), ("rear", b.raw[b.edge:]))

    def paint(self, byte: int):
        """Every guard <- `byte`; output and workspace payloads <- zero bytes; input payloads stay."""
        self.byte = int(byte) & 0xFF
        for b in self.bufs.values():
            for _side, g in self._guards(b):
                g.fill_(self.byte)
            if b.role != "in":
                b.raw[b.start:b.edge].zero_()

    # ---- checking -------------------------------------------------------------------------------------------------------------
    def check(self):
        """-> [Damage], one per damaged guard, in allocation order (front before rear); [] = clean."""
        assert self.byte is not None, "paint() first"
        guards = [(b, side, g) for b in self.bufs.values() for side, g in self._guards(b)]
        if not guards:
            return []
        counts = torch.stack([(g != self.byte).sum() for _b, _s, g in guards]).cpu().tolist()   # one transfer for all guards
        out = []
        for (b, side, g), n in zip(guards, counts):
            if n:
                first = int(torch.nonzero(g != self.byte)[0, 0])
                out.append(Damage(b.name, side, first if side == "rear" else first - b.start, int(n)))
        return out

    def assert_clean(self, entry: str, case):
        """Fails with e.g. "smtts_stitch case 3: `out` rear +0, 6 bytes"."""
        bad = self.check()
        assert not bad, report(entry, case, bad)


def report(entry: str, case, records) -> str:
    return f"{entry} case {case}: " + "; ".join(str(r) for r in records)
