"""CPU: the guarded allocator of the bounds tests (tests/helpers/guarded.py) on CPU tensors and plain torch writes from the test: what
it reports, where the guards lie, and that repainting restores a clean state.  No kernel runs here."""
import pytest
import torch

from tests.helpers.guarded import ALIGN, GUARD, Arena, Damage, report

G = 4096   # a small guard keeps these tests instant; the default is checked once below


def _arena():
    a = Arena("cpu", guard=G)
    a.put("x", torch.arange(7, dtype=torch.float32))
    a.alloc("out", (3, 5), torch.float32)
    a.alloc("pcm", 5, torch.int16)
    a.alloc("mask", (2, 3), torch.bool)
    a.workspace("ws", 1001)
    return a


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_untouched_arena_is_clean_and_payloads_are_as_promised(byte):
    a = _arena()
    a["out"].fill_(3.0)
    a["ws"].fill_(9)
    a.paint(byte)
    assert a.check() == []
    a.assert_clean("smtts_nothing", 0)
    assert torch.equal(a["x"], torch.arange(7, dtype=torch.float32))                     # inputs stay
    assert not a["out"].any() and not a["ws"].any() and not a["pcm"].any() and not a["mask"].any()   # outputs, workspaces: zero bytes
    # writing all of every payload leaves the guards alone
    a["out"].fill_(float("nan")); a["pcm"].fill_(-1); a["mask"].fill_(True); a["ws"].fill_(0xAB); a["x"].fill_(1.0)
    assert a.check() == []


def test_payloads_start_aligned_and_guards_have_their_width():
    a = _arena()
    for name, b in a.bufs.items():
        assert b.view.data_ptr() % ALIGN == 0, name
        assert b.view.data_ptr() == b.raw.data_ptr() + b.start
        assert b.start >= G and b.raw.numel() - b.edge >= G, name                          # at least `guard` bytes on either side
        assert b.edge - b.start == b.view.numel() * b.view.element_size(), name             # the rear guard begins at the exact byte
    assert Arena("cpu").guard == GUARD == 1 << 20
    v = Arena("cpu", guard=G).alloc("slab", 12, torch.float32, role="in", skew=4)           # 4-byte but not 16-byte aligned, on request
    assert v.data_ptr() % 16 == 4 and (v.data_ptr() - 4) % ALIGN == 0


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_single_bytes_are_reported_with_name_side_and_offset(byte):
    a = _arena()
    a.paint(byte)
    other = 0x5A
    b = a.bufs["out"]
    b.raw[b.edge] = other                      # rear +0: the byte right behind the payload
    assert a.check() == [Damage("out", "rear", 0, 1)]
    a.paint(byte)
    b.raw[b.start - 1] = other                 # front -1
    assert a.check() == [Damage("out", "front", -1, 1)]
    a.paint(byte)
    b.raw[b.raw.numel() - 1] = other           # the far end of the rear guard
    far = b.raw.numel() - 1 - b.edge
    assert far >= G - 1 and a.check() == [Damage("out", "rear", far, 1)]
    a.paint(byte)
    b.raw[0] = other                           # the far end of the front guard
    assert a.check() == [Damage("out", "front", -b.start, 1)]
    # several guards at once: one record each, in allocation order, the first changed byte and the count
    a.paint(byte)
    w = a.bufs["ws"]
    w.raw[w.edge + 2:w.edge + 8] = other
    b.raw[b.start - 3:b.start] = other
    assert a.check() == [Damage("out", "front", -3, 3), Damage("ws", "rear", 2, 6)]
    with pytest.raises(AssertionError) as e:
        a.assert_clean("smtts_stitch", 3)
    assert str(e.value).startswith("smtts_stitch case 3: `out` front -3, 3 bytes; `ws` rear +2, 6 bytes")
    assert report("smtts_stitch", 3, [Damage("out", "rear", 0, 6)]) == "smtts_stitch case 3: `out` rear +0, 6 bytes"
    assert str(Damage("pcm", "rear", 0, 1)) == "`pcm` rear +0, 1 byte"


@pytest.mark.parametrize("n,dtype", [(4099, torch.float32), (5, torch.int16), (1, torch.uint8), (3, torch.int64)])
def test_odd_sized_payload_has_its_rear_guard_at_the_exact_byte(n, dtype):
    a = Arena("cpu", guard=G)
    v = a.alloc("out", n, dtype)
    a.paint(0x00)
    flat = torch.zeros(n + 1, dtype=dtype)
    flat[n] = 1                                # one element past the end, written as the element type through the raw bytes
    b = a.bufs["out"]
    item = v.element_size()
    assert (b.raw.data_ptr() + b.edge) % ALIGN == n * item % ALIGN
    b.raw[b.edge:b.edge + item] = flat[n:].view(torch.uint8)
    (d,) = a.check()
    assert (d.name, d.side) == ("out", "rear") and 0 <= d.offset < item and d.offset + d.count <= item
    assert not v.any()                         # the payload itself is untouched
    v.fill_(1)                                 # ... and filling all of it does not reach the guard
    a.paint(0xFF)
    v.fill_(1)
    assert a.check() == []


def test_repainting_restores_a_clean_state_and_claim_moves_the_edge():
    a = _arena()
    a.paint(0xFF)
    for b in a.bufs.values():
        b.raw[b.edge] = 0
        b.raw[b.start - 1] = 0
    assert len(a.check()) == 2 * len(a.bufs)
    a.paint(0xFF)
    assert a.check() == []
    a.paint(0x00)
    assert a.check() == []
    # claim(): the checker is told the payload is shorter; a write into the rest of the true payload is then damage
    a.claim("ws", 500)
    a.paint(0x00)
    a["ws"][:500] = 7
    assert a.check() == []
    a["ws"][700:703] = 7
    assert a.check() == [Damage("ws", "rear", 200, 3)]
    with pytest.raises(AssertionError):
        Arena("cpu", guard=G).check()          # nothing painted yet
