"""smalltts_amd/operands.py on the CPU: the predicate and the shared checks take a wrong dtype, a wrong rank, a tensor that is not
contiguous, one on another device (the meta device serves), a misaligned view and None where it is allowed, and say what the engine's
methods always said.  The attention hook's precision comes back when its call raises (smalltts_amd/engine_hooks.py)."""
import numpy as np
import pytest
import torch

from smalltts_amd import operands as ops

CPU = torch.device("cpu")


def misaligned(t):
    raw = torch.zeros(t.numel() * t.element_size() + 8, dtype=torch.uint8)
    return raw[8:].view(t.dtype).view(t.shape)


def test_is_operand():
    t = torch.zeros(2, 5, 64)
    assert ops.is_operand(t, torch.float32, (2, None, 64), CPU)
    assert ops.is_operand(t, (torch.int32, torch.float32), (None, None, None), CPU)
    assert ops.is_operand(t, torch.float32, None, CPU)                                   # any rank
    assert ops.is_operand(torch.zeros(()), torch.float32, (), CPU)
    assert not ops.is_operand(t.double(), torch.float32, (2, 5, 64), CPU)                # dtype
    assert not ops.is_operand(t, torch.float32, (2, 5), CPU)                             # rank
    assert not ops.is_operand(t, torch.float32, (2, 5, 64, 1), CPU)
    assert not ops.is_operand(t, torch.float32, (2, 4, 64), CPU)                         # extent
    assert not ops.is_operand(t[:, :, ::2], torch.float32, (2, 5, 32), CPU)              # not contiguous
    assert not ops.is_operand(t.transpose(0, 1), torch.float32, (5, 2, 64), CPU)
    assert not ops.is_operand(torch.empty(2, 5, 64, device="meta"), torch.float32, (2, 5, 64), CPU)   # another device
    assert ops.is_operand(torch.empty(2, 5, 64, device="meta"), torch.float32, (2, 5, 64), torch.device("meta"))
    for other in (None, [0.0] * 4, np.zeros((2, 5, 64), np.float32), 3):
        assert not ops.is_operand(other, torch.float32, None, CPU)
    assert ops.is_operand(t, torch.float32, None, CPU, aligned=True)
    m = misaligned(t)
    assert m.is_contiguous() and m.data_ptr() % 16 == 8
    assert ops.is_operand(m, torch.float32, (2, 5, 64), CPU) and not ops.is_operand(m, torch.float32, (2, 5, 64), CPU, aligned=True)


def test_pool_and_slots():
    pool = torch.zeros(3, 256, dtype=torch.uint8)
    assert ops.pool_slots("m", CPU, pool, 256, "state", "decode_state") == 3
    text = "m: state must be a contiguous, 16-byte aligned uint8 (n_slots,256) tensor on the engine's device (decode_state())"
    for bad in (None, pool.int(), pool[0], pool[:, ::2].expand(3, 128), torch.zeros(3, 240, dtype=torch.uint8), misaligned(pool),
                torch.zeros(0, 256, dtype=torch.uint8), torch.empty(3, 256, dtype=torch.uint8, device="meta")):
        with pytest.raises(ValueError) as e:
            ops.pool_slots("m", CPU, bad, 256, "state", "decode_state")
        assert str(e.value) == text
    assert ops.distinct_slots("m", (2, np.int64(0)), 2, 3) == [2, 0]
    for bad, got in (([2, 2], "[2, 2]"), ([0, 3], "[0, 3]"), ([-1, 0], "[-1, 0]"), ([1], "[1]"), (None, "[]")):
        with pytest.raises(ValueError) as e:
            ops.distinct_slots("m", bad, 2, 3)
        assert str(e.value) == f"m: 2 distinct slots in [0, 3) wanted, got {got}"


def test_row_checks():
    assert ops.row_lengths("m", (40, 0), 2, 40) == [40, 0]
    for bad in ([41, 0], [-1, 0], [1]):
        with pytest.raises(ValueError, match=r"m: 2 lengths in \[0, 40\] wanted, got "):
            ops.row_lengths("m", bad, 2, 40)
    ops.per_row("m", 2, [5, 3])
    ops.per_row("m", 2, [5, 3], [0, 1], [4, 3])
    for args in ((2, [5]), (0, [])):
        with pytest.raises(ValueError, match="^m: one frame count per row$"):
            ops.per_row("m", *args)
    for args in ((2, [5], [0, 1], [4, 3]), (2, [5, 3], [0], [4, 3]), (2, [5, 3], [0, 1], [4, 3, 2]), (0, [], [], [])):
        with pytest.raises(ValueError, match="^m: one frame count and one token range per row$"):
            ops.per_row("m", *args)
    ops.frames_tokens("m", 1, 1)
    ops.frames_tokens("m", ops.ALIGN_MAX_FRAMES, ops.ALIGN_MAX_TOKENS)
    for n, p in ((0, 4), (226, 4), (5, 0), (5, 199)):
        with pytest.raises(ValueError) as e:
            ops.frames_tokens("m", n, p)
        assert str(e.value) == f"m: N = {n}, P = {p} outside the supported range N <= 225, P <= 198"


def test_fade_seg_gain_out():
    fade = torch.zeros(16)
    assert ops.fade_len("m", CPU, None) == 0 and ops.fade_len("m", CPU, fade) == 16 and ops.fade_len("m", CPU, fade.view(4, 4)) == 16
    assert ops.fade_len("m", CPU, torch.zeros(0, dtype=torch.int32)) == 0         # an empty table is no fade, whatever it is
    for bad in (fade.double(), torch.zeros(32)[::2], torch.empty(16, device="meta"), [0.5] * 16):
        with pytest.raises(ValueError, match="^m: fade must be a contiguous fp32 tensor on the engine's device$"):
            ops.fade_len("m", CPU, bad)
    seg, gain = torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2)
    ops.seg_gain("m", CPU, 2, seg, gain)
    ops.seg_gain("m", CPU, 2, seg, None)
    for bad in (None, seg.int(), seg[0], torch.zeros(2, 4, dtype=torch.int64)[:, ::2], torch.zeros(3, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"^m: seg must be a contiguous int64 \(B,2\) tensor on the engine's device$"):
            ops.seg_gain("m", CPU, 2, bad, gain)
    for bad in (gain.double(), gain[:, None], torch.zeros(3), torch.empty(2, device="meta")):
        with pytest.raises(ValueError, match=r"^m: gain must be a contiguous fp32 \(B,\) tensor on the engine's device, or None$"):
            ops.seg_gain("m", CPU, 2, seg, bad)
    ops.out_1d("m", CPU, torch.zeros(8))
    ops.out_1d("m", CPU, torch.zeros(0, dtype=torch.int16))
    for bad in (None, torch.zeros(8, dtype=torch.uint8), torch.zeros(2, 4), torch.zeros(16)[::2], torch.empty(8, device="meta")):
        with pytest.raises(ValueError, match="^m: out must be a contiguous 1-D fp32 or int16 tensor on the engine's device$"):
            ops.out_1d("m", CPU, bad)


def test_upload(monkeypatch):
    pinned = []
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda t: (pinned.append(t), t)[1])
    t = ops.upload([[5, 3], [0, 1]], np.int32, CPU)
    assert t.dtype == torch.int32 and t.tolist() == [[5, 3], [0, 1]] and pinned[0] is t
    u = ops.upload([np.asarray([2 ** 64 - 1, 7], np.uint64).view(np.int64), [5, 3]], np.int64, CPU)
    assert u.dtype == torch.int64 and u.tolist() == [[-1, 7], [5, 3]]
    assert ops.upload([2, 0], np.int64, CPU).tolist() == [2, 0]


def test_attention_hook_restores_the_precision_when_its_call_raises():
    from tests.helpers.engine_standin import StandinLib, make_engine, standin
    lib = StandinLib(fail=["smtts_test_attention_mfma"])
    with standin(lib, []):
        eng = make_engine(lib)
        q, w = torch.zeros(2, 5, 64), torch.zeros(8)
        with pytest.raises(RuntimeError, match="^test_attention: "):
            eng.test_attention(q, w, w, 1e-6, torch.zeros(5, 4), 4, 2, 8, mfma="img:bf16")
    made = [(name, args[1:]) for name, args in lib.calls if "precision" in name]
    assert made == [("smtts_set_site_precision", ["7", "1"]), ("smtts_set_precision", ["2"])]      # attn = bf16, then the preset again
