"""Writes tests/golden/g711_codes.npz: CPython's audioop.lin2ulaw(s, 2) and audioop.lin2alaw(s, 2) for every int16 s, in the order
s = -32768 .. 32767 (index s + 32768).  Needs a Python that still ships audioop (< 3.13); the tests read the file, not audioop.

    python tests/golden/make_g711_codes.py
"""
import audioop
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

if __name__ == "__main__":
    pcm = np.arange(-32768, 32768, dtype=np.int32).astype("<i2").tobytes()
    np.savez_compressed(os.path.join(HERE, "g711_codes.npz"),
                        mulaw=np.frombuffer(audioop.lin2ulaw(pcm, 2), np.uint8),
                        alaw=np.frombuffer(audioop.lin2alaw(pcm, 2), np.uint8),
                        python=np.array(sys.version.split()[0]))
