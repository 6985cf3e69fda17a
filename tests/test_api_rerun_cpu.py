"""CPU: the scenarios of tests/test_api_rerun_gpu.py against a stand-in engine, so that the host side of the fp16 range guard's re-run
(which record the rows, latents, windows, words and pieces are taken from) is checked wherever the suite runs.

The stand-in computes small deterministic tensors on the CPU.  Until its guard has fired its sampler clips its output, so the first
pass and the re-run differ in everything that is returned: latents, audio, speech windows, token spans.  Call A (the guard fires, the
call runs again) can therefore equal call B (one pass on the demoted engine) only if every returned element comes from the re-run.
"""
import contextlib
import warnings

import numpy as np
import pytest
import torch

from smalltts_amd import api
from tests import test_api_rerun_gpu as scenarios

HOP = api.HOP_SIZE


class StandInEngine:
    """The part of HipEngine that SmallTTS's synthesis calls use, on CPU tensors."""
    device = torch.device("cpu")

    def __init__(self, device_index=0):
        self.demoted = self.clamped = False
        self.reruns_under = []                   # the tuning in force at every sampler pass

    def load_state_dict(self, sd): pass
    def load_synthetic(self, *a, **kw): pass
    def finalize(self): pass
    def close(self): pass
    def use_workspace(self, slot): pass
    def has(self, part): return True
    def saturations(self, reset=True): return {"dit_block": 0}

    tuning = "latency"

    def set_tuning(self, mode):
        prev, self.tuning = self.tuning, mode
        return prev

    def cond_encode(self, ref, rs, ids, pm):
        self.P = int(np.asarray(ids).shape[1])
        return {"ref": float(np.asarray(ref, np.float32).sum()), "ids": float(np.asarray(ids).sum())}

    def voice_expand(self, voices):
        return {"voice": float(sum(float(v.k_ref.sum()) for v in voices))}

    def randn_rows(self, seeds, ns, steps, n_max=None):
        out = torch.zeros(steps, len(ns), max(ns) if n_max is None else n_max, 64)
        for b, (s, n) in enumerate(zip(seeds, ns)):
            out[:, b, :n] = torch.randn(steps, n, 64, generator=torch.Generator().manual_seed(int(s) % 2 ** 31))
        return out

    def sample(self, cache, mask, num_steps=4, noise=None, seed=0, align=None, **pins):
        self.reruns_under.append(self.tuning)
        B, N = mask.shape
        if noise is None:
            noise = torch.randn(num_steps, B, N, 64, generator=torch.Generator().manual_seed(int(seed) % 2 ** 31))
        x = torch.as_tensor(np.asarray(noise), dtype=torch.float32).sum(0) + sum(cache.values()) * 1e-3
        if not self.demoted:                     # "fp16 operands clamped": a clipped result, and the counter knows
            x, self.clamped = x.clamp(-1.0, 1.0), True
        x = x * torch.as_tensor(mask, dtype=torch.float32)[..., None]
        return x if align is None else (x, x[..., :1].abs().repeat(1, 1, self.P) + torch.arange(self.P))

    def align_path(self, mass, ns, p0, p1):
        spans = torch.full((mass.shape[0], mass.shape[2], 2), -1, dtype=torch.int32)
        for b, n in enumerate(ns):
            for t in range(p0[b], p1[b]):
                spans[b, t, 0], spans[b, t, 1] = int(mass[b, :n, t].sum().item() * 7 + t) % n, n - 1
        return spans, torch.zeros(len(ns))

    def codec_decode(self, x):
        B, N, _ = x.shape
        return (x.mean(-1)[:, :, None] * torch.linspace(0.5, 1.5, HOP)).reshape(B, 1, N * HOP).contiguous()

    def endpoints(self, audio, ns, ep, **kw):
        seg, gain = torch.zeros(len(ns), 2, dtype=torch.int64), torch.ones(len(ns))
        for b, n in enumerate(ns):
            h = int(audio[b, 0, :HOP * n].abs().sum().item() * 1000) % (HOP * n // 4)
            seg[b, 0], seg[b, 1], gain[b] = h, HOP * n - 2 * h, 0.5 + (h % 7) / 7
        return seg, gain, torch.zeros(len(ns), 1)

    def stitch(self, audio, ns, offsets, fade, out):
        for b, (n, o) in enumerate(zip(ns, offsets)):
            out[o:o + HOP * n] = audio[b, 0, :HOP * n]
        return out

    def stitch_seg(self, audio, seg, gain, offsets, fade, out):
        for b, o in enumerate(offsets):
            s, n = int(seg[b, 0]), int(seg[b, 1])
            out[o:o + n] = audio[b, 0, s:s + n] * (1.0 if gain is None else gain[b])
        return out

    def check_fp16_range(self, what=""):
        hit = ["dit_block"] if self.clamped and not self.demoted else []
        self.clamped = False
        if hit:
            self.demoted = True
            warnings.warn(f"fp16 range guard ({what}): site 'dit_block' clamped", RuntimeWarning)
        return hit


class _Stream:
    def __init__(self, *a): pass
    def wait_stream(self, other): pass


@pytest.mark.parametrize("scenario, args", [
    (scenarios.test_batch_with_trim_align_latents_and_raw_alignment, ()),
    (scenarios.test_plain_batch_with_ref_latents, ()),
    (scenarios.test_batches_in_flight, ()),
    (scenarios.test_long_with_segments_words_and_pieces, (scenarios.TRIM,)),
    (scenarios.test_long_with_segments_words_and_pieces, (None,)),
], ids=["batch-trim-align", "batch-plain", "batches-in-flight", "long-trim", "long-plain"])
def test_what_a_call_returns_after_the_guards_rerun_comes_from_the_rerun(monkeypatch, scenario, args):
    import smalltts_amd.engine
    made = []
    monkeypatch.setattr(smalltts_amd.engine, "HipEngine", lambda *a: made.append(StandInEngine()) or made[-1])
    monkeypatch.setattr(scenarios, "_outlier_dit_weights", lambda **kw: {})
    monkeypatch.setattr(api.SmallTTS, "encode_voice", lambda self, ref: api.Voice(self.engine, torch.ones(12, 1, 8, 10, 120),
                                                                                  torch.ones(12, 1, 8, 10, 120)))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: _Stream())
    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    monkeypatch.setattr(torch.cuda, "stream", lambda st: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda dev=None: None)
    scenario(*args)                                          # A warns and re-runs, B is silent, A == B bit for bit
    eng, = made
    assert eng.demoted and len(set(eng.reruns_under)) == 1, eng.reruns_under   # every pass under one tuning, as the scenario arranges
