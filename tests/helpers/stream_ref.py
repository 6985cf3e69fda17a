"""Numpy restatements for the streamed decode (tests/test_stream_cpu.py, tests/test_stream_gpu.py).

carry: what one carry_frames launch (smalltts_amd/csrc/codec_stream.hip) does to an image and the boundary's state blocks.
chunk_plan: how synthesize_stream cuts N latent frames into chunks."""
import numpy as np

PAD = 8   # frames in front of every row of a codec image = frames a boundary carries


def carry(img: np.ndarray, state: np.ndarray, T: int):
    """img (B, 8 + T, C), state (B, 8, C): row b's block of the boundary.  -> (img_new, state_new), copies:
    pad frame j <- state[j]; state_new[j] <- data frame T - 8 + j where that is >= 0, state[j + T] otherwise."""
    B, rows, C = img.shape
    assert rows == PAD + T and state.shape == (B, PAD, C) and T >= 1
    out, new = img.copy(), np.empty_like(state)
    out[:, :PAD] = state
    for j in range(PAD):
        t = T - PAD + j
        new[:, j] = img[:, PAD + t] if t >= 0 else state[:, j + T]
    return out, new


def carry_brute(history: np.ndarray, chunk: np.ndarray):
    """The definition carry() is checked against: history (B, n, C) = every frame of the image so far (n may be 0), chunk (B, T, C).
    -> (pad, state_new): the 8 frames in front of the chunk and the last 8 frames behind it, zeros where the utterance has none."""
    B, _, C = chunk.shape
    zeros = np.zeros((B, PAD, C), chunk.dtype)
    before = np.concatenate([zeros, history], axis=1)
    after = np.concatenate([before, chunk], axis=1)
    return before[:, -PAD:], after[:, -PAD:]


def chunk_plan(n: int, chunk_frames=(2, 4, 8, 16, 32)):
    """Chunk sizes of an utterance of n frames: chunk_frames in order, the last size repeated, the final chunk whatever is left."""
    sizes, k = [], 0
    while n > 0:
        c = min(int(chunk_frames[min(k, len(chunk_frames) - 1)]), n)
        sizes.append(c)
        n -= c
        k += 1
    return sizes
