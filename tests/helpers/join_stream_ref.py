"""Numpy restatement of the running join's contract (include/smalltts_hip.h smtts_join_stream), shared by the CPU test that
pins it to plan_packed + the stitch_seg restatement and by the GPU test that holds the kernel to it bit for bit.  numpy only."""
import numpy as np

from tests.helpers.longform_ref import pcm16_numpy


def clamp_seg(seg, row_stride):
    """smtts_stitch_seg's clamp of (start, n) into a row of row_stride samples; a negative n is an empty window."""
    out = []
    for s, n in np.asarray(seg, np.int64).reshape(-1, 2).tolist():
        s = min(max(s, 0), row_stride)
        out.append((s, max(0, min(n, row_stride - s))))
    return out


def window(audio, b, s, n, gain, fade):
    """One piece's samples: ((x * gain) * g), every step one fp32 multiply; gain None: no multiply."""
    row = np.array(audio[b, 0, s:s + n], np.float32)
    if gain is not None:
        row = row * np.float32(gain[b])
    Fb = min(len(fade), n // 2)
    if Fb:
        row[:Fb] = row[:Fb] * fade[:Fb]
        row[n - Fb:] = row[n - Fb:] * fade[:Fb][::-1]
    return row


def join_call(state, audio, seg, gain, fade, gap, pcm16=False, cap=None, last=False, slot=0):
    """One call.  state = (pos, k) -> (new state, chunk, off, rec, dtable): chunk = the samples the call appends (cut at `cap`), off the
    pieces' absolute positions, rec = (pos_before, pos_after, k_before, k_after), dtable = (slot, pos_before, length, last)."""
    pos0, k0 = int(state[0]), int(state[1])
    fade = np.asarray(fade if fade is not None else [], np.float32)
    dt = np.int16 if pcm16 else np.float32
    pos, k, parts, off = pos0, k0, [], []
    for b, (s, n) in enumerate(clamp_seg(seg, audio.shape[-1])):
        if n and k > 0:
            parts.append(np.zeros(gap, dt))
            pos += gap
        off.append(pos)
        if n:
            row = window(audio, b, s, n, gain, fade)
            parts.append(pcm16_numpy(row) if pcm16 else row)
            pos += n
            k += 1
    chunk = np.concatenate(parts) if parts else np.zeros(0, dt)
    assert chunk.shape[0] == pos - pos0
    if cap is not None:
        chunk = chunk[:cap]
    return (pos, k), chunk, off, (pos0, pos, k0, k), (int(slot), pos0, pos - pos0, int(bool(last)))
