"""CPU: the host side of streamed long-form synthesis: the numpy restatement of the running join run call by call against
plan_packed + the stitch_seg restatement run whole, the group schedule against brute force, the C ABI's bookkeeping, the chunked WAV
writer against wav_bytes, and the CLI's argument refusals."""
import itertools

import numpy as np
import pytest

from smalltts_amd import _lib
from smalltts_amd import audio as A
from smalltts_amd.api import plan_long, plan_packed, stream_groups
from tests.helpers import join_stream_ref as J
from tests.helpers.endpoint_ref import stitch_seg_numpy


def _calls(seed, sizes, row=700, empty_call=None):
    """Random windows for calls of `sizes` rows each; call number `empty_call` has only empty windows."""
    g = np.random.default_rng(seed)
    out = []
    for c, B in enumerate(sizes):
        audio = g.uniform(-1.5, 1.5, (B, 1, row)).astype(np.float32)
        seg = []
        for b in range(B):
            n = int(g.choice([0, 1, 5, 31, 255, 256, 257, row]))
            s = int(g.integers(0, row - n + 1))
            seg.append((s, 0 if c == empty_call else n))
        out.append((audio, seg, g.uniform(0.5, 2.0, B).astype(np.float32)))
    return out


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("gap, F, with_gain, empty_call", [(0, 0, False, None), (37, 16, True, None), (37, 16, False, 0), (5, 300, True, 1)])
def test_restatement_call_by_call_equals_plan_packed_and_stitch_seg_run_whole(pcm16, gap, F, with_gain, empty_call):
    calls = _calls(3 + gap + F, (3, 1, 4, 2), empty_call=empty_call)
    fade = (0.5 - 0.5 * np.cos(np.pi * (np.arange(F) + 0.5) / max(F, 1))).astype(np.float32)
    all_n = [n for _a, seg, _g in calls for _s, n in seg]
    offsets, S = plan_packed(all_n, gap * 1000.0 / 24000.0)
    dt = np.int16 if pcm16 else np.float32
    want = np.zeros(S, dt)
    state, chunks, offs, at = (0, 0), [], [], 0
    for audio, seg, gain in calls:
        gn = gain if with_gain else None
        stitch_seg_numpy(want, audio, seg, gn, offsets[at: at + len(seg)], fade)
        at += len(seg)
        before = state
        state, chunk, off, rec, dtable = J.join_call(state, audio, seg, gn, fade, gap, pcm16, last=at == len(all_n), slot=2)
        assert rec == (before[0], state[0], before[1], state[1]) and dtable == (2, before[0], chunk.shape[0], int(at == len(all_n)))
        chunks.append(chunk)
        offs += off
    assert offs == offsets and state == (S, sum(n > 0 for n in all_n))
    got = np.concatenate(chunks)
    assert got.dtype == dt and np.array_equal(got, want)


def test_restatement_clamps_like_stitch_seg_and_truncates_at_cap():
    audio = np.arange(20, dtype=np.float32).reshape(2, 1, 10)
    assert J.clamp_seg([(-3, 4), (8, 5), (12, 1), (2, -1)], 10) == [(0, 4), (8, 2), (10, 0), (2, 0)]
    state, chunk, off, rec, _d = J.join_call((7, 1), audio, [(8, 5), (0, 3)], None, None, 2, cap=6)
    assert chunk.tolist() == [0, 0, 8, 9, 0, 0] and off == [9, 13] and rec == (7, 16, 1, 3) and state == (16, 3)


def _brute(n, sizes, max_batch):
    out, i = [], 0
    for k in itertools.count():
        if i >= n:
            return out
        want = max_batch if sizes is None else min(sizes[k] if k < len(sizes) else sizes[-1], max_batch)
        out.append(list(range(i, min(i + want, n))))
        i += want


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 8, 15, 16, 40])
@pytest.mark.parametrize("sizes", [(1, 2, 4, 8), (1,), (3, 1), (16, 32), None])
@pytest.mark.parametrize("max_batch", [1, 2, 8])
def test_stream_groups_against_brute_force(n, sizes, max_batch):
    got = stream_groups(n, sizes, max_batch)
    assert got == _brute(n, sizes, max_batch)
    assert [i for g in got for i in g] == list(range(n)) and all(1 <= len(g) <= max_batch for g in got)
    if sizes is None:
        assert got == plan_long([1] * n, max_batch)[0]


def test_stream_groups_ramp_and_refusals():
    assert [len(g) for g in stream_groups(3, (1, 2, 4, 8), 8)] == [1, 2]                    # a ramp longer than the text
    assert [len(g) for g in stream_groups(40, (1, 2, 4, 8), 8)] == [1, 2, 4, 8, 8, 8, 8, 1]
    assert [len(g) for g in stream_groups(12, (1, 2, 4, 8), 3)] == [1, 2, 3, 3, 3]          # the max_batch cap
    for bad in ((), (0,), (2, -1)):
        with pytest.raises(ValueError):
            stream_groups(5, bad, 8)
    with pytest.raises(ValueError):
        stream_groups(5, (1,), 0)


def test_c_abi_bookkeeping():
    assert "smtts_join_stream" in _lib.SIGNATURES and "smtts_join_stream" in _lib.header_symbols() and _lib.ABI_VERSION == 11
    res, args = _lib.SIGNATURES["smtts_join_stream"]
    assert res is _lib.i32 and args[0] is _lib.vp and len(args) == 19
    assert "smtts_peek_saturations" in _lib.SIGNATURES and "smtts_peek_saturations" in _lib.header_symbols()


@pytest.mark.parametrize("encoding, sizes", [("pcm16", (0, 5, 1, 300)), ("mulaw", (7, 0, 2)), ("mulaw", (8, 2)), ("alaw", (3,)), ("f32", (4, 9))])
def test_wav_stream_writer_equals_wav_bytes_of_the_concatenation(tmp_path, encoding, sizes):
    g = np.random.default_rng(len(sizes))
    dt = A.DELIVER_DTYPES[encoding]
    chunks = [(g.standard_normal(n).astype(dt) if dt == np.float32 else g.integers(0, 200, n).astype(dt)) for n in sizes]
    path = tmp_path / "s.wav"
    with A.WavStreamWriter(str(path), 8000, encoding) as w:
        for c in chunks:
            w.write(c[None])
        with pytest.raises(ValueError):
            w.write(np.zeros(3, np.float64))
    assert path.read_bytes() == A.wav_bytes(np.concatenate(chunks), 8000, encoding)
    w.close()                                                                                 # closing twice is harmless
    with pytest.raises(ValueError):
        A.WavStreamWriter(str(path), 8000, "s16")


def test_wav_stream_writer_without_a_chunk_is_the_empty_wav(tmp_path):
    path = tmp_path / "e.wav"
    A.WavStreamWriter(str(path), 24000, "pcm16").close()
    assert path.read_bytes() == A.wav_bytes(np.zeros(0, np.int16), 24000, "pcm16")


def test_longform_cli_stream_arguments():
    from smalltts_amd.scripts import longform as L
    base = ["--wav", "r.wav", "--tokens-file", "t.txt", "--durations", "1"]
    a = L.parse_args(base)
    assert a.stream is False and a.batch_sizes is None
    assert L.parse_args(base + ["--stream"]).batch_sizes == (1, 2, 4, 8)
    assert L.parse_args(base + ["--stream", "--batch-sizes", "2,6"]).batch_sizes == (2, 6)
    assert L.parse_args(base + ["--stream", "--batch-sizes", "none"]).batch_sizes is None
    assert L.parse_args(base + ["--stream", "--words", "w.json", "--srt", "s.srt"]).stream is True
    for bad in (["--batch-sizes", "1,2"], ["--stream", "--batch-sizes", "0"], ["--stream", "--batch-sizes", "a,b"],
                ["--stream", "--batch-sizes", ""], ["--stream", "--rate", "8000", "--words", "w.json"],
                ["--stream", "--encoding", "mulaw", "--srt", "s.srt"]):
        with pytest.raises(SystemExit):
            L.parse_args(base + bad)
