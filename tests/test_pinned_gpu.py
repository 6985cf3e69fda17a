"""GPU: pinned sampling (smtts_sample_pinned: kernels.hip pin_renoise / pin_update) and what stands on it: HipEngine.sample(x_pin=,
pin=, start_step=), synthesize_batch(pins=), respeak, synthesize_long(return_pieces=) / render_long and the two CLIs.  Engine level:
the split-bf16 engine of tests/test_dit_gpu.py (DiT weights, the golden seed) and its bars against the oracle (TOL 1e-4 at split-bf16,
NORTH_STAR 1e-3 at the default precision); API level: the engine of tests/test_longform_gpu.py (seed 11, the tiny codec)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dit_oracle as O
from smalltts_amd.weights import CodecSpec
from tests.helpers import pinned_ref as PR

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_dit_gpu.py: split-bf16 sampler latents against the oracle, rel L2
NORTH_STAR = 1e-3   # ... and the default precision's bound
BARS = {"bf16x3": TOL, "f16": NORTH_STAR}
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
HOP = 3200


def snr_db(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return 10 * np.log10((ref ** 2).sum() / max(((got - ref) ** 2).sum(), 1e-300))


@pytest.fixture(scope="module")
def eng(golden_seed):
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(golden_seed, parts=("dit",))
    e.finalize()
    return e


class precision:
    def __init__(self, eng, prec):
        self.eng, self.prec = eng, prec

    def __enter__(self):
        self.eng.set_precision(self.prec)

    def __exit__(self, *a):
        self.eng.set_precision("bf16x3")


def _inputs(name):
    """-> dict(ref, ref_len, ids, ph_mask, mask, noise): the tiny case, a ragged (3,13,5,7) batch, the benchmark's (8,75,15,30)."""
    if name == "tiny":
        return PR.tiny_case()
    B, N, R, P = {"ragged": (3, 13, 5, 7), "bench": (8, 75, 15, 30)}[name]
    g = torch.Generator().manual_seed(21 if name == "ragged" else 22)
    ref = torch.randn(B, R, 64, generator=g)
    ids = torch.randint(1, 198, (B, P), generator=g)
    if name == "ragged":
        ref_len = torch.tensor([5, 3, 4])
        ph_mask = torch.arange(P)[None] < torch.tensor([7, 4, 6])[:, None]
        mask = torch.arange(N)[None] < torch.tensor([13, 9, 6])[:, None]
    else:
        ref_len, ph_mask, mask = torch.full((B,), R), torch.ones(B, P, dtype=torch.bool), torch.ones(B, N, dtype=torch.bool)
    ids = ids * ph_mask
    return dict(ref=ref, ref_len=ref_len, ids=ids, ph_mask=ph_mask, mask=mask, noise=torch.randn(4, B, N, 64, generator=g),
                fresh=torch.randn(B, N, 64, generator=g))


def _counts(eng, fn):
    eng.profile(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k["name"]: k["launches"] for k in eng.profile_report()}
    finally:
        eng.profile(False)


# ---- 1. nothing pinned: the plain sampler, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f16"])
@pytest.mark.parametrize("shape", ["tiny", "ragged", "bench"])
def test_nothing_pinned_is_the_plain_sampler_bit_for_bit(eng, shape, prec):
    c = _inputs(shape)
    with precision(eng, prec):
        cache = eng.cond_encode(c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
        for tuning in ("latency", "throughput"):
            prev = eng.set_tuning(tuning)
            try:
                for kw, pin in ((dict(noise=c["noise"]), torch.zeros_like(c["mask"])), (dict(seed=77), None)):   # host noise, Philox
                    x, steps = eng.sample(cache, c["mask"], num_steps=4, return_steps=True, **kw)
                    xp, stepsp = eng.sample(cache, c["mask"], num_steps=4, return_steps=True, x_pin=c["fresh"], pin=pin, **kw)
                    assert torch.equal(x, xp) and torch.equal(steps, stepsp), (shape, prec, tuning, sorted(kw))
                # the tap rides along unchanged
                x, mass = eng.sample(cache, c["mask"], num_steps=4, noise=c["noise"], align=True)
                xp, massp = eng.sample(cache, c["mask"], num_steps=4, noise=c["noise"], align=True, x_pin=c["fresh"])
                assert torch.equal(x, xp) and torch.equal(mass, massp)
                # the same launches, class by class: the two new classes stand where axpby (not a profiled class) ran
                plain = _counts(eng, lambda: eng.sample(cache, c["mask"], num_steps=4, seed=5))
                pinned = _counts(eng, lambda: eng.sample(cache, c["mask"], num_steps=4, seed=5, x_pin=c["fresh"]))
                assert pinned.pop("pin_renoise") == 4 and pinned.pop("pin_update") == 4
                plain.pop("axpby", None)
                assert pinned == plain and "pin_renoise" not in plain and "pin_update" not in plain
            finally:
                eng.set_tuning(prev)


# ---- 2. pins hold, the free frames follow the reference --------------------------------------------------------------------------
_RAGGED = {}


def _ragged_refs(w):
    """The ragged case, its pins and the oracle's runs (once per process): plain, pinned, pinned with row 0 fully pinned."""
    if not _RAGGED:
        c = _inputs("ragged")
        B, N = c["mask"].shape
        pin = torch.zeros(B, N, dtype=torch.bool)
        pin[0, ::2] = True                     # row 0: alternating frames
        pin[1, :3] = True                      # row 1: head and tail; the tail's bits run on behind the mask (9 frames)
        pin[1, 7:] = True
        pin[2, 6:] = True                      # row 2: free; bits behind its mask (6 frames) only
        full = pin.clone()
        full[0] = True                         # one run has a row fully pinned
        with torch.no_grad():
            cache = O.encode_conditions(w, c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
            run = lambda *a, **k: (lambda keep: (PR.sample_pinned(w, cache, c["ph_mask"], c["mask"], c["noise"], 4, *a, keep=keep), keep))([])
            _RAGGED.update(case=c, pin=pin, full=full, plain=run(), pinned=run(c["fresh"], pin), fullrow=run(c["fresh"], full),
                           late={(k, p): run(c["fresh"], pin if p else None, k) for k in (1, 2) for p in (False, True)})
    return _RAGGED


@pytest.mark.parametrize("prec", ["bf16x3", "f16"])
def test_pinned_frames_hold_and_free_frames_follow_the_reference(eng, dit_weights, prec):
    r = _ragged_refs(dit_weights)
    c, m = r["case"], r["case"]["mask"]
    with precision(eng, prec):
        cache = eng.cond_encode(c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
        x0 = eng.sample(cache, m, num_steps=4, noise=c["noise"]).cpu()
        e_plain = PR.rel(x0, r["plain"][0], m)
        for name, pin in (("pinned", r["pin"]), ("fullrow", r["full"])):
            x, steps = (t.cpu() for t in eng.sample(cache, m, num_steps=4, noise=c["noise"], return_steps=True, x_pin=c["fresh"], pin=pin))
            K = pin & m
            for got in [x] + list(steps):
                assert torch.equal(got[K], c["fresh"][K]), name          # bit for bit, in x_out and every step
            # bits behind the mask change nothing: the run with them cleared gives the same bits everywhere
            xc, stepsc = (t.cpu() for t in eng.sample(cache, m, num_steps=4, noise=c["noise"], return_steps=True, x_pin=c["fresh"], pin=K))
            assert torch.equal(x, xc) and torch.equal(steps, stepsc), name
            free = ~pin & m
            ox, osteps = r[name]
            errs = [PR.rel(x, ox, free)] + [PR.rel(steps[i], osteps[i], free) for i in range(4)]
            print(f"\n[pinned, {prec}, {name}] free frames vs reference: x {errs[0]:.3e}, steps {' '.join(f'{e:.3e}' for e in errs[1:])}; "
                  f"plain sampler at this shape {e_plain:.3e} (bar {BARS[prec]:.0e})")
            assert max(errs) < BARS[prec], (name, errs)
    assert e_plain < BARS[prec]


def test_tiny_case_the_pins_move_the_free_frames_on_the_gpu_too(eng, dit_weights):
    """The condition of the reference (tests/test_pinned_cpu.py) on the engine's own results, and the engine against the reference."""
    c, _cache, (oplain, _), (o1, _k1), (o2, _k2) = PR.tiny_refs(dit_weights)
    cache = eng.cond_encode(c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
    plain = eng.sample(cache, c["mask"], num_steps=4, noise=c["noise"]).cpu()
    set1 = eng.sample(cache, c["mask"], num_steps=4, noise=c["noise"], x_pin=plain, pin=c["pin"]).cpu()
    set2 = eng.sample(cache, c["mask"], num_steps=4, noise=c["noise"], x_pin=c["fresh"], pin=c["pin"]).cpu()
    free = PR.free_valid(c)
    e1, e2 = PR.rel(set1, plain, free), PR.rel(set2, set1, free)
    errs = [PR.rel(plain, oplain, c["mask"]), PR.rel(set1, o1, free), PR.rel(set2, o2, free)]
    print(f"\n[pinned tiny] free frames: set 1 vs plain {e1:.3e}, set 2 vs set 1 {e2:.3e}; vs reference: plain {errs[0]:.3e}, "
          f"set 1 {errs[1]:.3e}, set 2 {errs[2]:.3e}")
    assert e1 > 1e-2 and e2 > 1e-2
    assert max(errs) < TOL


# ---- 3. rows do not see each other's pins; repeatable ----------------------------------------------------------------------------
def test_a_rows_pins_do_not_touch_the_other_rows_and_runs_repeat(eng, dit_weights):
    r = _ragged_refs(dit_weights)
    c = r["case"]
    cache = eng.cond_encode(c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
    for tuning in ("latency", "throughput"):
        prev = eng.set_tuning(tuning)
        try:
            a = eng.sample(cache, c["mask"], num_steps=4, seed=9, x_pin=c["fresh"], pin=r["pin"])
            again = eng.sample(cache, c["mask"], num_steps=4, seed=9, x_pin=c["fresh"], pin=r["pin"])
            other = r["pin"].clone()
            other[1] = ~other[1]
            fresh2 = c["fresh"].clone()
            fresh2[1] += 1.0
            b = eng.sample(cache, c["mask"], num_steps=4, seed=9, x_pin=fresh2, pin=other)
        finally:
            eng.set_tuning(prev)
        assert torch.equal(a, again)
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1]), tuning


# ---- 4. late starts, refused arguments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "f16"])
def test_late_start_follows_the_reference(eng, dit_weights, prec):
    r = _ragged_refs(dit_weights)
    c, m = r["case"], r["case"]["mask"]
    with precision(eng, prec):
        cache = eng.cond_encode(c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
        for (k, pinned), (ox, osteps) in r["late"].items():
            pin = r["pin"] if pinned else None
            x, steps = (t.cpu() for t in eng.sample(cache, m, num_steps=4, noise=c["noise"], return_steps=True, x_pin=c["fresh"], pin=pin,
                                                    start_step=k))
            assert not steps[:k].any() and len(osteps) == 4 - k        # the slots below the start are zeros
            assert torch.equal(x, steps[3])
            sel = (~pin & m) if pinned else m
            errs = [PR.rel(steps[i], osteps[i - k], sel) for i in range(k, 4)]
            print(f"\n[late start {k}, {'pins' if pinned else 'no pins'}, {prec}] vs reference: {' '.join(f'{e:.3e}' for e in errs)}")
            assert PR.rel(x, ox, sel) < BARS[prec] and max(errs) < BARS[prec], (k, pinned, errs)
            if pinned:
                K = pin & m
                assert all(torch.equal(steps[i][K], c["fresh"][K]) for i in range(k, 4))
        # Philox: step i draws stream i whatever the start: the run from the plain run's own step 1 ends where the plain run ends
        x, steps = eng.sample(cache, m, num_steps=4, seed=31, return_steps=True)
        late = eng.sample(cache, m, num_steps=4, seed=31, x_pin=steps[1], start_step=2)
        assert torch.equal(late, x)
        # the tap's mean counts the steps that ran: flagged 0 and 3 from start 2 = flagged 3 alone
        _x, m1 = eng.sample(cache, m, num_steps=4, seed=31, x_pin=steps[1], start_step=2, align=type("A", (), dict(layers=None, heads=None, steps=(0, 3)))())
        _x, m2 = eng.sample(cache, m, num_steps=4, seed=31, x_pin=steps[1], start_step=2, align=True)
        assert torch.equal(m1, m2)


def test_refused_arguments_enqueue_nothing(eng, dit_weights):
    c = _inputs("ragged")
    cache = eng.cond_encode(c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
    B, N = c["mask"].shape
    R, P = 5, 7
    dev = eng.device
    mask, noise, x_pin, pin = c["mask"].to(dev), c["noise"].to(dev), c["fresh"].to(dev), torch.zeros(B, N, dtype=torch.bool, device=dev)
    odd = torch.zeros(B * N * 64 + 1, device=dev)[1:].view(B, N, 64)          # a 4-byte aligned view
    mass = torch.zeros(B, N, P, device=dev)
    ws = torch.empty(int(eng.lib.smtts_sample_workspace_bytes(eng.h, B, N, R, P, 4, 1)), dtype=torch.uint8, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    flags0 = (C.c_uint8 * 4)(1, 0, 0, 0)

    def call(mode=0, cfg=0, x_pin=x_pin, pin=pin, start=0, tap=None, text_mass=None):
        x = torch.full((B, N, 64), 7.0, device=dev)
        eng.profile(True)
        try:
            rc = eng.lib.smtts_sample_pinned(eng.h, eng._stream(), mode, 4, cfg, 2.0, 1.5, p(mask), p(cache["k_ref"]), p(cache["v_ref"]),
                                             p(cache["ref_mask"]), p(cache["k_text"]), p(cache["v_text"]), p(cache["ph_mask"]), B, N, R, P,
                                             p(noise), C.c_uint64(0), p(x), None, p(ws), ws.numel(),
                                             C.cast(tap, C.c_void_p) if tap is not None else None, 0xFFF, 0xFF, p(text_mass), p(x_pin),
                                             p(pin), start)
            torch.cuda.synchronize()
            launched = eng.profile_report()
        finally:
            eng.profile(False)
        return rc, launched, bool((x == 7.0).all()), eng.lib.smtts_last_error(eng.h).decode()

    rc, launched, untouched, _ = call()
    assert rc == 0 and launched and not untouched                              # the harness itself: a valid call runs
    bad = [dict(mode=1), dict(cfg=1), dict(start=-1), dict(start=4), dict(x_pin=None, pin=None, start=1), dict(x_pin=None),
           dict(x_pin=odd), dict(start=1, tap=flags0, text_mass=mass)]
    for kw in bad:
        rc, launched, untouched, msg = call(**kw)
        assert rc == 1 and launched == [] and untouched and msg, (kw.keys(), rc, launched, msg)
    # the Python surface says so before the call, with ValueError
    m = c["mask"]
    for kw in (dict(pin=c["mask"]), dict(start_step=1), dict(x_pin=c["fresh"], start_step=4), dict(x_pin=c["fresh"], start_step=-1),
               dict(x_pin=c["fresh"][:, :5]), dict(x_pin=c["fresh"].double()), dict(x_pin=c["fresh"], pin=m[:, :5]),
               dict(x_pin=c["fresh"], pin=m.to(torch.uint8)), dict(x_pin=c["fresh"], mode="ode")):
        with pytest.raises(ValueError):
            eng.sample(cache, m, num_steps=4, noise=None if kw.get("mode") else c["noise"], **kw)


# ---- API level ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def api_eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(SEED, parts=("dit", "decoder", "encoder"), codec_spec=SPEC)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def tts(api_eng):
    from smalltts_amd.api import SmallTTS
    return SmallTTS(engine=api_eng, seed=1)


@pytest.fixture(scope="module")
def refs():
    g = np.random.default_rng(0)
    return [g.standard_normal((r, 64)).astype(np.float32) for r in (5, 9, 7)]


@pytest.fixture(scope="module")
def voices(tts, refs):
    return [tts.encode_voice(r) for r in refs]


TOKS = [[1, 2, 3, 4], [10, 20, 30, 40, 50, 60], [7] * 9]
NS = [7, 16, 11]
SPANS = [(2, 5), (6, 10), None]          # the frames regenerated per row; row 2 rides along unpinned


def _check_rows(orig, orig_lat, got, got_lat):
    for b, fr in enumerate(SPANS):
        if fr is None:                    # the same seed, no pins: the row as it was
            assert np.array_equal(got_lat[b], orig_lat[b]) and np.array_equal(got[b], orig[b])
            continue
        f0, f1 = fr
        assert got_lat[b].shape == orig_lat[b].shape and got[b].shape == orig[b].shape
        assert np.array_equal(got_lat[b][:f0], orig_lat[b][:f0]) and np.array_equal(got_lat[b][f1:], orig_lat[b][f1:])   # kept: bit for bit
        assert not np.array_equal(got_lat[b][f0:f1], orig_lat[b][f0:f1])
        assert np.array_equal(got[b][:, : HOP * f0], orig[b][:, : HOP * f0])     # the causal codec: the audio in front is untouched
        assert not np.array_equal(got[b][:, HOP * f0:], orig[b][:, HOP * f0:])


def _pins(orig_lat):
    from smalltts_amd.api import splice_pins
    return [None if fr is None else splice_pins(orig_lat[b], *fr) for b, fr in enumerate(SPANS)]


def test_synthesize_batch_pins(tts, refs, voices):
    for kw in (dict(ref_latents=refs), dict(ref_latents=None, voices=voices)):
        ref = kw.pop("ref_latents")
        orig, orig_lat = tts.synthesize_batch(ref, TOKS, None, frames=NS, seeds=[5, 6, 7], return_latents=True, **kw)
        pins = _pins(orig_lat)
        got, got_lat = tts.synthesize_batch(ref, TOKS, None, frames=NS, seeds=[15, 16, 7], return_latents=True, pins=pins, **kw)
        _check_rows(orig, orig_lat, got, got_lat)
    # explicit noise instead of seeds
    g = np.random.default_rng(3)
    noise, noise2 = (g.standard_normal((4, 3, 16, 64)).astype(np.float32) for _ in range(2))
    noise2[:, 2] = noise[:, 2]
    orig, orig_lat = tts.synthesize_batch(refs, TOKS, None, frames=NS, noise=noise, return_latents=True)
    got, got_lat = tts.synthesize_batch(refs, TOKS, None, frames=NS, noise=noise2, return_latents=True, pins=_pins(orig_lat))
    _check_rows(orig, orig_lat, got, got_lat)
    # trim: the rows come back as their speech windows, cut out of the very same audio; align: the words come back
    kw = dict(frames=NS, voices=voices, seeds=[15, 16, 7], return_latents=True, pins=_pins(orig_lat))
    full, full_lat = tts.synthesize_batch(None, TOKS, None, **kw)
    cut, cut_lat, words = tts.synthesize_batch(None, TOKS, None, trim=True, align=True, **kw)
    from smalltts_amd.api import token_groups
    assert [[(i, k) for i, k, _s, _e in w] for w in words] == [[(i, g[0]) for i, g in enumerate(token_groups(t))] for t in TOKS]
    for b in range(3):
        assert np.array_equal(cut_lat[b], full_lat[b])
        n = cut[b].shape[1]
        assert 0 <= n <= full[b].shape[1]
        if n:
            starts = [s for s in np.flatnonzero(full[b][0] == cut[b][0, 0]) if s + n <= full[b].shape[1]]
            assert any(np.array_equal(full[b][0, s:s + n], cut[b][0]) for s in starts), b
    # a late start keeps the pins too, and needs latents everywhere
    lat3 = [(orig_lat[b], np.zeros(NS[b], bool)) if p is None else (orig_lat[b], p[1]) for b, p in enumerate(_pins(orig_lat))]
    got, got_lat = tts.synthesize_batch(refs, TOKS, None, frames=NS, seeds=[15, 16, 17], return_latents=True, pins=lat3, start_step=2)
    for b, fr in enumerate(SPANS):
        if fr is not None:
            assert np.array_equal(got_lat[b][:fr[0]], orig_lat[b][:fr[0]]) and np.array_equal(got_lat[b][fr[1]:], orig_lat[b][fr[1]:])
            assert not np.array_equal(got_lat[b][fr[0]:fr[1]], orig_lat[b][fr[0]:fr[1]])


def test_respeak_same_and_changed_length(tts, voices, refs):
    toks, n, (f0, f1) = TOKS[1], 16, (6, 10)
    (orig,), (lat,) = tts.synthesize_batch(None, [toks], None, frames=[n], voices=[voices[1]], seeds=[6], return_latents=True)
    audio, new = tts.respeak(toks, lat, (f0, f1), voice=voices[1], seed=60)
    assert audio.shape == (1, HOP * n) and new.shape == (n, 64)
    assert np.array_equal(new[:f0], lat[:f0]) and np.array_equal(new[f1:], lat[f1:]) and not np.array_equal(new[f0:f1], lat[f0:f1])
    assert np.array_equal(audio[:, : HOP * f0], orig[:, : HOP * f0]) and not np.array_equal(audio[:, HOP * f0:], orig[:, HOP * f0:])
    again = tts.respeak(toks, lat, (f0, f1), voice=voices[1], seed=60)
    assert np.array_equal(again[0], audio) and np.array_equal(again[1], new)
    for m in (2, 7):                          # another length, another text: the tail moves with it
        audio, new, words = tts.respeak(toks, lat, (f0, f1), ref_latents=refs[1], new_tokens=[10, 20, 33, 34, 50, 60], new_frames=m,
                                        seed=61, align=True)
        n2 = n - (f1 - f0) + m
        assert audio.shape == (1, HOP * n2) and new.shape == (n2, 64) and [w[1] for w in words] == ["punct", "word"]
        assert np.array_equal(new[:f0], lat[:f0]) and np.array_equal(new[f0 + m:], lat[f1:])
    # the last step alone: nearly a no-op by the schedule (alpha(0) = 1, sigma(0) = 3.1e-5); kept frames exact as ever
    _a, near = tts.respeak(toks, lat, (f0, f1), voice=voices[1], seed=62, start_step=3)
    assert np.array_equal(near[:f0], lat[:f0]) and np.array_equal(near[f1:], lat[f1:])
    print(f"\n[respeak] start_step = 3: free frames moved by rel L2 {PR.rel(near[f0:f1], lat[f0:f1], np.ones((f1 - f0, 64), bool)):.3e}")


def test_render_long_reproduces_the_take_and_a_respoken_piece_leaves_the_rest(tts, voices):
    from smalltts_amd.api import Endpointing, Piece, piece_seed
    g = np.random.default_rng(12)
    durs = [1.0, 2.2, 1.5, 0.7, 3.0, 1.2, 2.0, 0.5, 1.8, 2.6, 0.9]
    ns = [max(1, int(d * 7.5)) for d in durs]
    toks = [[int(t) for t in g.integers(1, 198, size=int(g.integers(3, 20)))] for _ in durs]
    voice = voices[1]
    kw = dict(token_lists=toks, durations=durs, seed=3)
    plain = tts.synthesize_long(voice, **kw)
    out, segs, pieces = tts.synthesize_long(voice, return_segments=True, return_pieces=True, **kw)
    assert np.array_equal(out, plain)                                          # asking for the pieces changes nothing
    assert len(pieces) == 11 and all(isinstance(p, Piece) for p in pieces)
    assert [p.latents.shape for p in pieces] == [(n, 64) for n in ns] and [p.seed for p in pieces] == [piece_seed(3, i) for i in range(11)]
    assert [list(p.tokens) for p in pieces] == toks and all(p.prefix_len == 0 and p.spans is None for p in pieces)
    got, gsegs = tts.render_long(pieces, return_segments=True)
    assert np.array_equal(got, out) and gsegs == segs
    assert np.array_equal(tts.render_long([p.latents for p in pieces]), out)   # plain arrays do as well
    assert np.array_equal(tts.render_long(pieces, pcm16=True), tts.synthesize_long(voice, pcm16=True, **kw))
    ep = Endpointing(level_dbfs=-20.0)
    tout, tsegs, tpieces, = tts.synthesize_long(voice, trim=ep, return_segments=True, return_pieces=True, **kw)
    tgot, tgsegs = tts.render_long(tpieces, trim=ep, return_segments=True)
    assert np.array_equal(tgot, tout) and tgsegs == tsegs
    assert all(np.array_equal(a.latents, b.latents) for a, b in zip(pieces, tpieces))
    # with words the pieces carry their spans; the waveform is the same
    wout, _wsegs, _words, wpieces = tts.synthesize_long(voice, return_segments=True, return_words=True, return_pieces=True, **kw)
    assert np.array_equal(wout, out) and all(p.spans.shape == (len(p.tokens), 2) for p in wpieces)

    # piece 4 (the longest of its group) spoken again over frames [f0, f1), same length: nothing else moves
    f0, f1 = 9, 15
    p4 = pieces[4]
    _a, lat4 = tts.respeak(p4.tokens, p4.latents, (f0, f1), voice=voice, seed=99)
    take2 = list(pieces)
    take2[4] = Piece(p4.tokens, 0, lat4, 99)
    out2, segs2 = tts.render_long(take2, return_segments=True)
    assert segs2 == segs and out2.shape == out.shape
    for i, (off, n, _s, _g) in enumerate(segs):
        if i != 4:
            assert np.array_equal(out2[0, off:off + n], out[0, off:off + n]), i
    off, n = segs[4][:2]
    assert np.array_equal(out2[0, off:off + HOP * f0], out[0, off:off + HOP * f0])
    assert not np.array_equal(out2[0, off + HOP * f0:off + n], out[0, off + HOP * f0:off + n])
    # ... another length: the group's batch changes shape, the unchanged pieces are held to the batch-shape bar (80 dB)
    _a, lat4 = tts.respeak(p4.tokens, p4.latents, (f0, f1), voice=voice, seed=99, new_frames=3)
    take3 = list(pieces)
    take3[4] = Piece(p4.tokens, 0, lat4, 99)
    out3, segs3 = tts.render_long(take3, return_segments=True)
    shift = HOP * (3 - (f1 - f0))
    assert out3.shape[1] == out.shape[1] + shift
    worst = 1e9
    for i, ((off, n, _s, _g), (off3, n3, _s3, _g3)) in enumerate(zip(segs, segs3)):
        assert off3 == off + (shift if i > 4 else 0) and n3 == n + (shift if i == 4 else 0)
        if i != 4:
            worst = min(worst, snr_db(out3[0, off3:off3 + n3], out[0, off:off + n]))
    print(f"\n[render_long] a piece of another length: the unchanged pieces agree to {worst:.1f} dB at worst")
    assert worst > 80.0


def test_both_clis_end_to_end(tmp_path):
    """longform --take --words, then respeak --groups on the take: the wav and the updated take come out, everything in front of the
    re-spoken piece is the same PCM."""
    from smalltts_amd.api import load_take
    from smalltts_amd.audio import read_wav, write_wav_pcm16
    sr = 16000
    t = np.arange(int(0.9 * sr)) / sr
    write_wav_pcm16(str(tmp_path / "ref.wav"), 0.5 * np.sin(2 * np.pi * 440 * t), sr)
    with open(tmp_path / "tokens.txt", "w") as f:
        f.write("1,2,3,4,5,6,7,8\n10,20,30,40\n5,9,14,33,41,14,77,120,3\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--wav", str(tmp_path / "ref.wav"), "--weights", "synthetic:3"]
    r = subprocess.run([sys.executable, "-m", "smalltts_amd.scripts.longform", "--tokens-file", str(tmp_path / "tokens.txt"), "--durations",
                        "1.0,0.6,1.5", "--out", str(tmp_path / "long.wav"), "--seed", "0", "--gap-ms", "100", "--take", str(tmp_path / "take.npz"),
                        "--words", str(tmp_path / "words.json")] + common, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    pieces, join = load_take(tmp_path / "take.npz")
    assert [p.latents.shape[0] for p in pieces] == [7, 4, 11] and join["gap_ms"] == 100.0 and not join["trim"]
    assert all(p.spans is not None and p.spans.shape == (len(p.tokens), 2) for p in pieces)
    r = subprocess.run([sys.executable, "-m", "smalltts_amd.scripts.respeak", "--take", str(tmp_path / "take.npz"), "--piece", "1", "--groups",
                        "1:2", "--seed", "5", "--out", str(tmp_path / "out" / "fixed.wav"), "--take-out", str(tmp_path / "take2.npz")] + common,
                       cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    a, rate = read_wav(str(tmp_path / "long.wav"))
    b, rate2 = read_wav(str(tmp_path / "out" / "fixed.wav"))
    assert rate == rate2 == 24000 and a.shape == b.shape == (HOP * (7 + 4 + 11) + 2 * 2400,)
    assert np.array_equal(a[: HOP * 7 + 2400], b[: HOP * 7 + 2400]) and not np.array_equal(a, b)
    pieces2, join2 = load_take(tmp_path / "take2.npz")
    assert join2 == join and pieces2[1].seed == 5 and pieces2[1].spans is not None
    assert all(np.array_equal(pieces2[i].latents, pieces[i].latents) for i in (0, 2)) and not np.array_equal(pieces2[1].latents, pieces[1].latents)
