"""GPU: every product entry point of the C ABI between guard bands (tests/helpers/guarded.py).

Every input, every output and the workspace of a call is a view into an allocation of its own with 1 MiB of guard in front and behind,
the workspace exactly as large as its *_workspace_bytes call says.  Each case runs twice, the guards painted 0x00 and then 0xFF (NaN
as fp32, -1 as int64, "true" as a mask byte), and asserts
  a. no write outside: no guard byte changed in either run;
  b. no read outside that matters: the outputs of the two runs are the same bytes, and the same bytes as the HipEngine wrapper's
     (where the wrapper cannot express the call, a plain restatement stands in and the test says so);
  c. the size contract: a call with ws_bytes - 1 is refused as "workspace too small" and touches neither outputs nor guards.
Nothing here can fault: every byte a guard watches belongs to the test's own allocation.  The engines are the ones the existing tests
build (tests/test_fullsize_gpu.py: golden seed, DiT + full-spec codec; tests/test_longform_gpu.py: seed 11, the tiny codec), at both
presets and both tunings, which select different kernels, ring depths, the LN fold and the stage chain."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import dit_oracle as O
from smalltts_amd.weights import CodecSpec
from tests.helpers import endpoint_ref as ER
from tests.helpers.guarded import Arena, report
from tests.helpers.longform_ref import stitch_numpy

pytestmark = pytest.mark.gpu
SPEC = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))  # hop 3200, tiny channels
SEED = 11
PRESETS = ("f16", "bf16x3")
TUNINGS = ("latency", "throughput")
F32, I64, I32, I16, U8, BOOL = torch.float32, torch.int64, torch.int32, torch.int16, torch.uint8, torch.bool


@pytest.fixture(scope="module")
def full(golden_seed):
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(golden_seed, parts=("dit", "decoder", "encoder"))
    e.finalize()
    return e


@pytest.fixture(scope="module")
def tiny():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0, "bf16x3")
    e.load_synthetic(SEED, parts=("dit", "decoder", "encoder"), codec_spec=SPEC)
    e.finalize()
    return e


class mode:
    """The engine at a preset and a tuning for the length of a test; split-bf16 / latency (what the fixtures start with) afterwards."""

    def __init__(self, eng, preset="bf16x3", tuning="latency"):
        self.eng, self.preset, self.tuning = eng, preset, tuning

    def __enter__(self):
        self.eng.set_precision(self.preset)
        self.eng.set_tuning(self.tuning)

    def __exit__(self, *a):
        self.eng.set_precision("bf16x3")
        self.eng.set_tuning("latency")


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def same(a, b):
    """The same bytes (NaNs included)."""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(-1).view(U8), b.view(-1).view(U8))


class Call:
    """One call of one entry point with all its buffers in an arena.  fn(ws_pointer, ws_bytes) -> rc makes the call (entries without
    a workspace ignore both)."""

    def __init__(self, eng, entry, case):
        self.eng, self.entry, self.case = eng, entry, case
        self.a = Arena(eng.device)
        self.outs, self.ws, self.ws_bytes, self.fn = [], None, 0, None

    def inp(self, name, t, skew=0):
        return self.a.put(name, t, skew=skew)

    def out(self, name, shape, dtype=F32):
        self.outs.append(name)
        return self.a.alloc(name, shape, dtype)

    def workspace(self, nbytes, slack=0):
        """Exactly what the size query returned (slack: the misaligned-workspace cases need room to move the pointer)."""
        self.ws_bytes = int(nbytes)
        self.ws = self.a.workspace("ws", self.ws_bytes + slack)
        return self.ws

    def invoke(self, ws_ptr=None, ws_bytes=None):
        if self.ws is not None and ws_ptr is None:
            ws_ptr, ws_bytes = self.ws.data_ptr(), self.ws_bytes
        rc = self.fn(C.c_void_p(ws_ptr) if ws_ptr is not None else None, ws_bytes)
        torch.cuda.synchronize()
        return rc

    def error(self):
        return self.eng.lib.smtts_last_error(self.eng.h).decode()

    def payload_bytes(self, name):
        b = self.a.bufs[name]
        return b.raw[b.start:b.start + b.nbytes]

    def run(self):
        """Checks a, the two-paintings half of b and c; -> {output name: tensor} of the first run."""
        snaps = []
        for byte in (0x00, 0xFF):
            self.a.paint(byte)
            rc = self.invoke()
            assert rc == 0, f"{self.entry} case {self.case}: rc {rc}: {self.error()}"
            self.a.assert_clean(self.entry, f"{self.case} (guards 0x{byte:02X})")
            snaps.append({n: self.a[n].clone() for n in self.outs})
        for n in self.outs:
            assert same(snaps[0][n], snaps[1][n]), (f"{self.entry} case {self.case}: `{n}` differs between guards painted 0x00 and 0xFF: "
                                                    f"something read outside a buffer reaches the result")
        if self.ws is not None:
            self.refused(self.ws.data_ptr(), self.ws_bytes - 1, "workspace too small")
        return snaps[0]

    def refused(self, ws_ptr, ws_bytes, needle):
        """The call is refused with `needle` in the message; outputs, workspace and guards stay as painted."""
        self.a.paint(0xFF)
        rc = self.invoke(ws_ptr, ws_bytes)
        msg = self.error()
        assert rc != 0 and needle in msg, f"{self.entry} case {self.case}: rc {rc}, message {msg!r} (expected {needle!r})"
        self.a.assert_clean(self.entry, f"{self.case} (refused: {needle})")
        for n in self.outs + ([] if self.ws is None else ["ws"]):
            assert not bool(self.payload_bytes(n).any()), f"{self.entry} case {self.case}: the refused call wrote `{n}`"

    def matches(self, got, want: dict):
        for n, w in want.items():
            assert same(got[n], w), f"{self.entry} case {self.case}: `{n}` differs from the HipEngine wrapper's"


# ---- DiT inputs -------------------------------------------------------------------------------------------------------------------------
DIT_SHAPES = [(1, 1, 1, 1), (3, 13, 5, 7), (1, 65, 3, 2), (2, 75, 15, 30)]   # the smallest call; ragged; one row past a 64-row tile; M = 150


def dit_inputs(B, N, R, P):
    g = torch.Generator().manual_seed(1000 * B + N)
    if (B, N, R, P) == (3, 13, 5, 7):          # the ragged lengths of tests/test_pinned_gpu.py::_inputs("ragged")
        rl, pl, nl = [5, 3, 4], [7, 4, 6], [13, 9, 6]
    else:                                       # the last row of a batch is short on every axis
        rl, pl, nl = ([R] * (B - 1) + [max(1, R // 3)], [P] * (B - 1) + [max(1, P // 2)], [N] * (B - 1) + [max(1, (2 * N) // 3)]) if B > 1 \
            else ([R], [P], [N])
    ph_mask = torch.arange(P)[None] < torch.tensor(pl)[:, None]
    c = dict(ref=torch.randn(B, R, 64, generator=g), ref_len=torch.tensor(rl), ids=torch.randint(1, 198, (B, P), generator=g) * ph_mask,
             ph_mask=ph_mask, mask=torch.arange(N)[None] < torch.tensor(nl)[:, None], noise=torch.randn(4, B, N, 64, generator=g),
             fresh=torch.randn(B, N, 64, generator=g), t=torch.rand(B, generator=g))
    pin = torch.zeros(B, N, dtype=torch.bool)
    if (B, N) == (3, 13):                       # the pins of tests/test_pinned_gpu.py: their bits run on behind the mask
        pin[0, ::2] = True
        pin[1, :3] = True
        pin[1, 7:] = True
        pin[2, 6:] = True
    else:
        pin[:, ::3] = True
    c["pin"] = pin
    return c


CACHE_KEYS = ("k_ref", "v_ref", "ref_mask", "k_text", "v_text", "ph_mask")


def cond_call(eng, c, case, slack=0):
    B, R, _ = c["ref"].shape
    P = c["ids"].shape[1]
    k = Call(eng, "smtts_cond_encode", case)
    ref, rl, ids, pm = k.inp("ref", c["ref"]), k.inp("ref_len", c["ref_len"].to(I64)), k.inp("ids", c["ids"].to(I64)), k.inp("ph_mask", c["ph_mask"])
    kr, vr, rm = k.out("k_ref", (12, B, 8, R, 120)), k.out("v_ref", (12, B, 8, R, 120)), k.out("ref_mask", (B, R), BOOL)
    kt, vt = k.out("k_text", (12, B, 8, P, 120)), k.out("v_text", (12, B, 8, P, 120))
    rs, mem = k.out("ref_seq", (B, R, 960)), k.out("phoneme_mem", (B, P, 960))
    k.workspace(eng.lib.smtts_cond_workspace_bytes(eng.h, B, R, P), slack)
    k.fn = lambda ws, n: eng.lib.smtts_cond_encode(eng.h, eng._stream(), p(ref), p(rl), p(ids), p(pm), B, R, P, p(kr), p(vr), p(rm), p(kt),
                                                   p(vt), ws, n, p(rs), p(mem))
    return k


def put_cache(k, cache):
    return {n: k.inp(n, cache[n]) for n in CACHE_KEYS}


def denoise_call(eng, c, cache, case, slack=0):
    B, N = c["mask"].shape
    R, P = cache["k_ref"].shape[3], cache["k_text"].shape[3]
    k = Call(eng, "smtts_denoise_step", case)
    x, m, t = k.inp("x_t", c["fresh"]), k.inp("mask", c["mask"]), k.inp("t", c["t"])
    g = put_cache(k, cache)
    v = k.out("velocity", (B, N, 64))
    k.workspace(eng.lib.smtts_denoise_workspace_bytes(eng.h, B, N, R, P), slack)
    k.fn = lambda ws, n: eng.lib.smtts_denoise_step(eng.h, eng._stream(), p(x), p(m), p(t), p(g["k_ref"]), p(g["v_ref"]), p(g["ref_mask"]),
                                                    p(g["k_text"]), p(g["v_text"]), p(g["ph_mask"]), None, B, N, R, P, p(v), ws, n)
    return k


def sample_call(eng, c, cache, case, kind="plain", ode=False, steps=4, start_step=0, slack=0):
    """kind "plain" smtts_sample, "align" smtts_sample_align (the tap on the last step), "pinned" smtts_sample_pinned (+ the tap).
    ode: the teacher mode with cfg = 1: mask and cache carry 3 B rows, the noise comes from the device's Philox."""
    B, N = c["mask"].shape
    R, P = cache["k_ref"].shape[3], cache["k_text"].shape[3]
    cfg = int(ode)
    k = Call(eng, {"plain": "smtts_sample", "align": "smtts_sample_align", "pinned": "smtts_sample_pinned"}[kind], case)
    m = k.inp("mask", c["mask"].repeat(3, 1) if cfg else c["mask"])
    g = put_cache(k, cache)
    nz = None if ode else k.inp("noise", c["noise"][:steps])
    x, so = k.out("x_out", (B, N, 64)), k.out("steps_out", (steps, B, N, 64))
    mass = k.out("text_mass", (B, N, P)) if kind != "plain" else None
    xp, pin = (k.inp("x_pin", c["fresh"]), k.inp("pin", c["pin"])) if kind == "pinned" else (None, None)
    k.workspace(eng.lib.smtts_sample_workspace_bytes(eng.h, B, N, R, P, steps, cfg), slack)
    head = lambda ws, n: (eng.h, eng._stream(), int(ode), steps, cfg, 2.0, 1.5, p(m), p(g["k_ref"]), p(g["v_ref"]), p(g["ref_mask"]), p(g["k_text"]),
                          p(g["v_text"]), p(g["ph_mask"]), B, N, R, P, p(nz), C.c_uint64(77), p(x), p(so), ws, n)
    if kind == "plain":
        k.fn = lambda ws, n: eng.lib.smtts_sample(*head(ws, n))
    elif kind == "align":
        k.fn = lambda ws, n: eng.lib.smtts_sample_align(*head(ws, n), None, 0xFFF, 0xFF, p(mass))       # tap_steps NULL: the last step
    else:
        k.fn = lambda ws, n: eng.lib.smtts_sample_pinned(*head(ws, n), None, 0xFFF, 0xFF, p(mass), p(xp), p(pin), start_step)
    return k


def wrapper_cache(eng, c):
    return eng.cond_encode(c["ref"], c["ref_len"], c["ids"], c["ph_mask"])


def cfg_cache(eng, c):
    r3, l3, i3, p3 = O.cfg_conditions(c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
    return eng.cond_encode(r3, l3, i3, p3)


# ---- DiT cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", TUNINGS)
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("shape", DIT_SHAPES)
def test_cond_encode_and_denoise_step(full, shape, preset, tuning):
    c = dit_inputs(*shape)
    case = f"{shape} {preset} {tuning}"
    with mode(full, preset, tuning):
        k = cond_call(full, c, case)
        got = k.run()
        want = full.cond_encode(c["ref"], c["ref_len"], c["ids"], c["ph_mask"], debug=True)
        k.matches(got, {n: want[n] for n in ("k_ref", "v_ref", "ref_mask", "k_text", "v_text", "ref_seq", "phoneme_mem")})
        d = denoise_call(full, c, want, case)
        got = d.run()
        d.matches(got, {"velocity": full.denoise_step(c["fresh"], c["mask"], c["t"], want)})


@pytest.mark.parametrize("tuning", TUNINGS)
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("shape", [(3, 13, 5, 7), (2, 75, 15, 30)])
def test_sample_dmd_and_teacher(full, shape, preset, tuning):
    c = dit_inputs(*shape)
    case = f"{shape} {preset} {tuning}"
    with mode(full, preset, tuning):
        cache = wrapper_cache(full, c)
        k = sample_call(full, c, cache, case + " dmd 4 steps")
        got = k.run()
        x, steps = full.sample(cache, c["mask"], num_steps=4, noise=c["noise"], return_steps=True)
        k.matches(got, {"x_out": x, "steps_out": steps})
        cache3 = cfg_cache(full, c)                      # the teacher / ODE mode with cfg: three times the rows
        k = sample_call(full, c, cache3, case + " ode cfg 2 steps", ode=True, steps=2)
        got = k.run()
        x, steps = full.sample(cache3, c["mask"], num_steps=2, mode="ode", cfg=True, seed=77, return_steps=True)
        k.matches(got, {"x_out": x, "steps_out": steps})


@pytest.mark.parametrize("tuning", TUNINGS)
@pytest.mark.parametrize("preset", PRESETS)
def test_sample_align_and_pinned(full, preset, tuning):
    """The text-mass tap with text_mass guarded, and the pinned sampler with the ragged pins (their bits run on behind the mask), from
    step 0 and from step 2."""
    c = dit_inputs(3, 13, 5, 7)
    case = f"(3, 13, 5, 7) {preset} {tuning}"
    with mode(full, preset, tuning):
        cache = wrapper_cache(full, c)
        k = sample_call(full, c, cache, case, kind="align")
        got = k.run()
        x, steps, mass = full.sample(cache, c["mask"], num_steps=4, noise=c["noise"], return_steps=True, align=True)
        k.matches(got, {"x_out": x, "steps_out": steps, "text_mass": mass})
        for start in (0, 2):
            k = sample_call(full, c, cache, f"{case} start_step {start}", kind="pinned", start_step=start)
            got = k.run()
            x, steps, mass = full.sample(cache, c["mask"], num_steps=4, noise=c["noise"], return_steps=True, align=True, x_pin=c["fresh"],
                                         pin=c["pin"], start_step=start)
            k.matches(got, {"x_out": x, "steps_out": steps, "text_mass": mass})
            K = (c["pin"] & c["mask"]).to(full.device)
            assert torch.equal(got["x_out"][K], c["fresh"].to(full.device)[K])          # the pinned frames hold, as on the wrapper's path


@pytest.mark.parametrize("N,P", [(1, 1), (13, 7), (225, 198)])
def test_align_path(full, N, P):
    B = 3
    g = torch.Generator().manual_seed(N)
    mass = torch.rand(B, N, P, generator=g)
    mass = mass / mass.sum(-1, keepdim=True)
    ns, p0, p1 = [N, (N + 1) // 2, 0], [0, min(1, P - 1), 0], [P, P, max(1, P // 2)]       # a full row, a prefix skipped, an empty row
    k = Call(full, "smtts_align_path", f"N {N} P {P}")
    m = k.inp("mass", mass)
    tab = [k.inp(n, torch.tensor(v, dtype=I32)) for n, v in (("n_len", ns), ("p0", p0), ("p1", p1))]
    spans, score = k.out("spans", (B, P, 2), I32), k.out("score", (B,))
    k.fn = lambda ws, n: full.lib.smtts_align_path(full.h, full._stream(), p(m), B, N, P, p(tab[0]), p(tab[1]), p(tab[2]), p(spans), p(score))
    got = k.run()
    ws, wsc = full.align_path(mass.to(full.device), ns, p0, p1)
    k.matches(got, {"spans": ws, "score": wsc})


# ---- codec cases ------------------------------------------------------------------------------------------------------------------------
def decode_call(eng, lat, case, slack=0):
    B, T, _ = lat.shape
    k = Call(eng, "smtts_codec_decode", case)
    x = k.inp("latents", lat)
    audio = k.out("audio", (B, 1, eng.hop * T))
    k.workspace(eng.lib.smtts_decode_workspace_bytes(eng.h, B, T), slack)
    k.fn = lambda ws, n: eng.lib.smtts_codec_decode(eng.h, eng._stream(), p(x), B, T, p(audio), ws, n)
    return k


def encode_call(eng, audio, case, slack=0):
    B, _, S = audio.shape
    k = Call(eng, "smtts_codec_encode", case)
    x = k.inp("audio", audio)
    lat = k.out("latents", (B, S // eng.hop, 64))
    k.workspace(eng.lib.smtts_encode_workspace_bytes(eng.h, B, S), slack)
    k.fn = lambda ws, n: eng.lib.smtts_codec_encode(eng.h, eng._stream(), p(x), B, S, p(lat), ws, n)
    return k


CODEC_DECODE = [("tiny", 1, 1), ("tiny", 3, 2), ("tiny", 2, 5), ("tiny", 2, 75), ("full", 1, 1), ("full", 2, 5)]
CODEC_ENCODE = [("tiny", 1, 1), ("tiny", 2, 1), ("tiny", 1, 5), ("tiny", 2, 5), ("full", 1, 2)]      # (spec, B, S / hop)


@pytest.mark.parametrize("tuning", TUNINGS)
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("spec,B,T", CODEC_DECODE)
def test_codec_decode(request, spec, B, T, preset, tuning):
    eng = request.getfixturevalue(spec)
    lat = torch.randn(B, T, 64, generator=torch.Generator().manual_seed(40 + T))
    with mode(eng, preset, tuning):
        k = decode_call(eng, lat, f"{spec} B {B} T {T} {preset} {tuning}")
        got = k.run()
        k.matches(got, {"audio": eng.codec_decode(lat)})


@pytest.mark.parametrize("tuning", TUNINGS)
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("spec,B,hops", CODEC_ENCODE)
def test_codec_encode(request, spec, B, hops, preset, tuning):
    eng = request.getfixturevalue(spec)
    audio = torch.randn(B, 1, hops * 3200, generator=torch.Generator().manual_seed(7 + hops)) * 0.3
    with mode(eng, preset, tuning):
        assert eng.hop == 3200
        k = encode_call(eng, audio, f"{spec} B {B} S {hops} hop {preset} {tuning}")
        got = k.run()
        k.matches(got, {"latents": eng.codec_encode(audio)})


# ---- small kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4099])
def test_randn(tiny, n):
    k = Call(tiny, "smtts_randn", f"n {n}")
    out = k.out("out", (n,))
    k.fn = lambda ws, nb: tiny.lib.smtts_randn(tiny.h, tiny._stream(), p(out), n, C.c_uint64(1234), C.c_uint64(3))
    k.matches(k.run(), {"out": tiny.randn(n, 1234, 3)})


def test_randn_rows(tiny):
    steps, B, Nmax, ns, seeds = 4, 3, 13, (13, 9, 0), (1234, 2 ** 63 - 5, 99)
    k = Call(tiny, "smtts_randn_rows", "4 steps, n (13, 9, 0) of 13")
    sd, n = k.inp("seeds", torch.tensor(seeds, dtype=I64)), k.inp("n", torch.tensor(ns, dtype=I64))
    out = k.out("out", (steps, B, Nmax, 64))
    k.fn = lambda ws, nb: tiny.lib.smtts_randn_rows(tiny.h, tiny._stream(), p(out), p(sd), p(n), steps, B, Nmax)
    got = k.run()
    k.matches(got, {"out": tiny.randn_rows(seeds, ns, steps, n_max=Nmax)})
    assert not bool(got["out"][:, 2].any()) and not bool(got["out"][:, 1, 9:].any())


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("n_in", [1, 7, 4410])
@pytest.mark.parametrize("sr", [44100, 16000])
def test_resample_poly(tiny, sr, n_in, channels):
    from smalltts_amd.audio import _sinc_kernel
    g = math.gcd(sr, 24000)
    down, up = sr // g, 24000 // g
    bank, width = _sinc_kernel(down, up)
    n_out = int(math.ceil(up * n_in / down))
    xs = torch.randn(channels, n_in, generator=torch.Generator().manual_seed(n_in)) * 0.5
    k = Call(tiny, "smtts_resample_poly", f"{sr} -> 24000, n_in {n_in}, {channels} channel(s)")
    x, b = k.inp("x", xs), k.inp("bank", torch.from_numpy(bank))
    y = k.out("y", (channels, n_out))
    k.fn = lambda ws, nb: tiny.lib.smtts_resample_poly(tiny.h, tiny._stream(), p(x), channels, n_in, p(b), up, down, bank.shape[1], width, p(y),
                                                       n_out)
    k.matches(k.run(), {"y": tiny.resample(xs, sr)})


@pytest.mark.parametrize("n", [1, 5001])
def test_pcm16(tiny, n):
    xs = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.6          # some samples beyond +-1: the clamp works
    k = Call(tiny, "smtts_pcm16", f"n {n}")
    x = k.inp("x", xs)
    y = k.out("y", (n,), I16)
    k.fn = lambda ws, nb: tiny.lib.smtts_pcm16(tiny.h, tiny._stream(), p(x), n, p(y))
    k.matches(k.run(), {"y": tiny.pcm16(xs)})


@pytest.mark.parametrize("skewed", [False, True])
@pytest.mark.parametrize("Rmax", [5, 7])
def test_voice_expand(tiny, Rmax, skewed):
    """R_b = (5, 3, 4) into Rmax = 5 and 7; skewed: voice 1's k slab at an address that is 4-byte but not 16-byte aligned (the kernel's
    scalar path), still between guards.  The wrapper always takes Rmax = max R_b, so at Rmax = 7 the plain definition stands in: copies
    in front, zeros behind."""
    Rs, B = (5, 3, 4), 3
    g = torch.Generator().manual_seed(Rmax)
    k = Call(tiny, "smtts_voice_expand", f"Rmax {Rmax}{' skewed slab' if skewed else ''}")
    slabs = [(k.inp(f"k{b}", torch.randn(12, 1, 8, R, 120, generator=g), skew=4 if skewed and b == 1 else 0),
              k.inp(f"v{b}", torch.randn(12, 1, 8, R, 120, generator=g))) for b, R in enumerate(Rs)]
    assert slabs[1][0].data_ptr() % 16 == (4 if skewed else 0)
    table = k.inp("table", torch.tensor([[ks.data_ptr(), vs.data_ptr(), R] for (ks, vs), R in zip(slabs, Rs)], dtype=I64))
    kr, vr, rm = k.out("k_ref", (12, B, 8, Rmax, 120)), k.out("v_ref", (12, B, 8, Rmax, 120)), k.out("ref_mask", (B, Rmax), BOOL)
    k.fn = lambda ws, nb: tiny.lib.smtts_voice_expand(tiny.h, tiny._stream(), p(table), B, Rmax, p(kr), p(vr), p(rm))
    got = k.run()
    want = {"k_ref": torch.zeros_like(kr), "v_ref": torch.zeros_like(vr), "ref_mask": torch.zeros_like(rm)}
    for b, ((ks, vs), R) in enumerate(zip(slabs, Rs)):
        want["k_ref"][:, b, :, :R], want["v_ref"][:, b, :, :R], want["ref_mask"][b, :R] = ks[:, 0], vs[:, 0], True
    for n, w in want.items():
        assert same(got[n], w), (k.case, n)
    if Rmax == 5:
        k.matches(got, tiny.voice_expand(slabs))


def _stitch_rows(row_stride, lens, seed):
    g = np.random.default_rng(seed)
    audio = (g.standard_normal((len(lens), 1, row_stride)) * 0.6).astype(np.float32)      # some samples beyond +-1: the PCM clamp works
    return audio


# (row_stride, lens, offsets, F): odd row lengths at odd offsets, the last row ending exactly on out's last sample; more than one block
# of 256 quads; no fade table
STITCH = [(37, (37, 22, 5), (3, 45, 70), 6), (2051, (2051, 1030, 7), (1, 2055, 3090), 120), (19, (19, 1), (0, 19), 0)]


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("case", range(len(STITCH)))
def test_stitch(tiny, case, pcm16):
    """The wrapper takes whole codec frames per row, so the numpy restatement (tests/helpers/longform_ref.py, bit for bit) stands in."""
    stride, lens, offs, F = STITCH[case]
    out_n = offs[-1] + lens[-1]
    audio = _stitch_rows(stride, lens, case)
    fade = (0.5 - 0.5 * np.cos(np.pi * (np.arange(F) + 0.5) / max(F, 1))).astype(np.float32)
    k = Call(tiny, "smtts_stitch", f"{case} {'pcm16' if pcm16 else 'fp32'}")
    a, ln, of = k.inp("audio", torch.from_numpy(audio)), k.inp("len", torch.tensor(lens, dtype=I64)), k.inp("off", torch.tensor(offs, dtype=I64))
    fd = k.inp("fade", torch.from_numpy(fade)) if F else None
    out = k.out("out", (out_n,), I16 if pcm16 else F32)
    k.fn = lambda ws, nb: tiny.lib.smtts_stitch(tiny.h, tiny._stream(), p(a), len(lens), stride, p(ln), p(of), p(fd), F, p(out), out_n, int(pcm16))
    got = k.run()
    want = stitch_numpy(np.zeros(out_n, np.int16 if pcm16 else np.float32), audio, lens, offs, fade)
    assert np.array_equal(got["out"].cpu().numpy(), want), k.case


@pytest.mark.parametrize("with_gain", [False, True])
@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("case", range(len(STITCH)))
def test_stitch_seg(tiny, case, pcm16, with_gain):
    """Windows at odd starts; the last one runs past the end of out by two samples, which the kernel drops."""
    stride, lens, offs, F = STITCH[case]
    seg = [(min(1, n - 1), n - min(1, n - 1)) for n in lens[:-1]] + [(0, lens[-1])]
    out_n = offs[-1] + lens[-1] - min(2, lens[-1])
    audio = _stitch_rows(stride, lens, 10 + case)
    gain = np.random.default_rng(case).uniform(0.2, 3.0, len(lens)).astype(np.float32) if with_gain else None
    fade = (0.5 - 0.5 * np.cos(np.pi * (np.arange(F) + 0.5) / max(F, 1))).astype(np.float32)
    k = Call(tiny, "smtts_stitch_seg", f"{case} {'pcm16' if pcm16 else 'fp32'}{' gain' if with_gain else ''}")
    a, sg, of = k.inp("audio", torch.from_numpy(audio)), k.inp("seg", torch.tensor(seg, dtype=I64)), k.inp("off", torch.tensor(offs, dtype=I64))
    gn = k.inp("gain", torch.from_numpy(gain)) if with_gain else None
    fd = k.inp("fade", torch.from_numpy(fade)) if F else None
    out = k.out("out", (out_n,), I16 if pcm16 else F32)
    k.fn = lambda ws, nb: tiny.lib.smtts_stitch_seg(tiny.h, tiny._stream(), p(a), len(lens), stride, p(sg), p(gn), p(of), p(fd), F, p(out), out_n,
                                                    int(pcm16))
    got = k.run()
    want = ER.stitch_seg_numpy(np.zeros(out_n + 2, np.int16 if pcm16 else np.float32), audio, seg, gain, offs, fade)[:out_n]
    assert np.array_equal(got["out"].cpu().numpy(), want), k.case
    w = tiny.stitch_seg(a, sg, gn, offs, fd, torch.zeros(out_n, dtype=out.dtype, device=tiny.device))
    k.matches(got, {"out": w})


class Params:
    def __init__(self, **kw):
        self.p = ER.params(**kw)

    def kernel_params(self):
        return self.p


@pytest.mark.parametrize("target_rms", [0.0, 0.25])
@pytest.mark.parametrize("W", [16, 240, 304, 4096])     # the frame sizes of tests/test_endpoint_gpu.py
def test_endpoints(tiny, W, target_rms):
    """row_stride larger than every length; lengths 0, 1, W - 1, W, W + 1, 3 W + 5; NaN behind every row's length (nothing there is
    read); without (target_rms = 0: gain 1) and with levelling.  e and pk are scratch AND output, written for the row's own frames
    and untouched behind: the wrapper's are compared there.  The ABI has no call without the gain pointer: NULL is refused."""
    lens = [0, 1, W - 1, W, W + 1, 3 * W + 5]
    B, stride = len(lens), 3 * W + 5 + 3
    Fmax = (stride + W - 1) // W
    g = np.random.default_rng(W)
    rows = [((g.standard_normal(max(n, 1)) * 0.1).astype(np.float32), n) for n in lens]
    audio, _ = ER.pad_batch(rows, np.nan, stride)
    ep = Params(W=W, min_run=1, lead=W // 2, tail=W, target_rms=np.float32(target_rms))
    q = ep.kernel_params()
    k = Call(tiny, "smtts_endpoints", f"W {W} target_rms {target_rms}")
    a, ln = k.inp("audio", torch.from_numpy(audio)), k.inp("len", torch.tensor(lens, dtype=I64))
    e, pk, seg, gain = k.out("e", (B, Fmax)), k.out("pk", (B, Fmax)), k.out("seg", (B, 2), I64), k.out("gain", (B,))
    args = lambda gp: (tiny.h, tiny._stream(), p(a), B, stride, p(ln), W, float(q["rel_pow"]), float(q["floor_pow"]), int(q["min_run"]),
                       int(q["lead"]), int(q["tail"]), float(q["target_rms"]), float(q["peak_limit"]), float(q["max_gain"]), p(e), p(pk), p(seg), gp)
    k.fn = lambda ws, nb: tiny.lib.smtts_endpoints(*args(p(gain)))
    got = k.run()
    wseg, wgain, we, wpk = tiny.endpoints(a, None, ep, lens=lens, return_peaks=True)
    k.matches(got, {"seg": wseg, "gain": wgain})
    for b, n in enumerate(lens):
        F = (n + W - 1) // W
        assert same(got["e"][b, :F], we[b, :F]) and same(got["pk"][b, :F], wpk[b, :F]), (k.case, b)
        assert not bool(got["e"][b, F:].any()) and not bool(got["pk"][b, F:].any()), (k.case, b)          # untouched behind
    assert bool(torch.isfinite(got["e"]).all()) and bool(torch.isfinite(got["gain"]).all())
    k.fn = lambda ws, nb: tiny.lib.smtts_endpoints(*args(None))
    k.refused(None, None, "bad arguments")


# ---- the workspace alignment contract ---------------------------------------------------------------------------------------------------
def _ws_calls(full, tiny, slack):
    """The smallest case of every entry that takes a workspace."""
    c = dit_inputs(3, 13, 5, 7)
    cache = wrapper_cache(full, c)
    lat = torch.randn(1, 1, 64, generator=torch.Generator().manual_seed(1))
    audio = torch.randn(1, 1, 3200, generator=torch.Generator().manual_seed(2)) * 0.3
    return [cond_call(full, c, "misaligned", slack), denoise_call(full, c, cache, "misaligned", slack),
            sample_call(full, c, cache, "misaligned", slack=slack), sample_call(full, c, cache, "misaligned", kind="align", slack=slack),
            sample_call(full, c, cache, "misaligned", kind="pinned", slack=slack), decode_call(tiny, lat, "misaligned", slack),
            encode_call(tiny, audio, "misaligned", slack)]


def test_misaligned_workspace_is_refused_before_anything_runs(full, tiny):
    """include/smalltts_hip.h: a workspace must be 256-byte aligned.  The arena holds ws_bytes + 256, so the moved span stays inside the
    payload; the pointer advanced by 4 and by 16 bytes is refused with a message that names the alignment, and outputs, workspace and
    guards stay untouched.  (Nothing else is tried with a misaligned workspace: without the check it can abort the process.)"""
    for k in _ws_calls(full, tiny, 256):
        assert k.ws.data_ptr() % 256 == 0
        for adv in (4, 16):
            k.case = f"workspace + {adv}"
            k.refused(k.ws.data_ptr() + adv, k.ws_bytes, "256-byte aligned")
        k.a.paint(0x00)                                   # the same buffers, the pointer where it belongs: the call runs
        assert k.invoke() == 0, (k.entry, k.error())
        k.a.assert_clean(k.entry, "aligned again")


# ---- the checker sees a kernel's write: one permanent self-test on the device -----------------------------------------------------------
def test_self_test_a_write_behind_a_moved_edge_is_reported(full):
    """smtts_sample at (3, 13, 5, 7) with the checker told that the workspace ends half-way: the engine still gets all of it, every
    byte is the test's own, and check() must report the kernels' writes into the second half as damage of `ws`'s rear guard."""
    c = dit_inputs(3, 13, 5, 7)
    k = sample_call(full, c, wrapper_cache(full, c), "self-test")
    k.a.claim("ws", k.ws_bytes // 2)
    k.a.paint(0x00)
    assert k.invoke() == 0, k.error()
    bad = k.a.check()
    print("\n[self-test] " + report(k.entry, k.case, bad))
    assert len(bad) == 1 and bad[0].name == "ws" and bad[0].side == "rear" and bad[0].count > 0, bad
    assert 0 <= bad[0].offset < k.ws_bytes - k.ws_bytes // 2                   # inside the true workspace: nothing went past its end
    with pytest.raises(AssertionError, match=r"smtts_sample case self-test: `ws` rear \+\d+, \d+ bytes"):
        k.a.assert_clean(k.entry, k.case)
