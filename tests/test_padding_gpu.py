"""GPU: nothing behind a mask or a length, and no other row of the batch, reaches the visible part of a row's result.  Bit for bit.

The cases, the hidden regions and the three classes of hidden values (zero / draw / large) are tests/helpers/padding_cases.py's; the
CPU oracles have the property exactly on the same cases (tests/test_padding_cpu.py).  Here every masked or batched entry of the C ABI
runs with `zero`, then `draw`, then `large` behind its masks: the same shape, the same settings, the same buffers at the same
addresses, outputs and workspace zero-filled before every run, so the launches are the same and a visible element may not move a bit.
No tolerance anywhere in this file, and no exception: no dependence on hidden values was found, by design or otherwise (DESIGN §9
records what was found; a case held to the fp64 oracle instead would have to be argued there and listed here by name).

Per (entry, shape, preset) one test; inside it three settings (latency tuning, throughput tuning, latency tuning without the LN fold;
the codec also with the fused FFN / mixer kernels off) x the classes.  Also asserted: every output is finite everywhere, hidden rows
included; the saturation counters and the range report of `draw` are those of `zero` (another draw of the same distribution must not
move a guard; for `large` the counts are printed, not asserted: whether a clamp in a row behind the mask should count is product
behaviour); text_mass is exactly 0 outside (visible frame, visible text column).  Row isolation: every other row of the batch
redrawn, lengths and masks kept.  Liveness: with one hidden element declared visible the same comparison must FAIL, or a test that
never uploaded the painted tensor would pass.

No NaN / Inf (the reference itself spreads a hidden NaN through 0 x NaN in P V), ids in range, full-size buffers, aligned pointers:
nothing here can fault."""
import ctypes as C
from contextlib import contextmanager

import pytest
import torch

from tests.helpers import padding_cases as PC

pytestmark = pytest.mark.gpu
PRESETS = ("f16", "bf16x3")
SETTINGS = ("latency", "throughput", "latency, LN fold off")
SHAPES = tuple(PC.DIT_SHAPES)
F32, I64, BOOL, U8 = torch.float32, torch.int64, torch.bool, torch.uint8
MASS_AXES = "(row, frame, text column)"
LARGE_CLAMPS = {}          # test id -> {setting: {site: count}} of class `large`: recorded and printed, not asserted

_engines = {}


def engine(kind, preset, golden_seed=None):
    """One engine per (weights, preset), built once per module: "dit" = the golden-seed synthetic DiT, else a codec spec of PC.CODEC_SPECS."""
    if (kind, preset) not in _engines:
        from smalltts_amd.engine import HipEngine
        e = HipEngine(0, preset)
        if kind == "dit":
            e.load_synthetic(golden_seed, parts=("dit",))
        else:
            e.load_synthetic(PC.CODEC_SEED, parts=("decoder", "encoder"), codec_spec=PC.CODEC_SPECS[kind])
        e.finalize()
        _engines[(kind, preset)] = e
    return _engines[(kind, preset)]


@contextmanager
def setting(eng, name, fused=True):
    try:
        if name == "throughput":
            eng.set_tuning("throughput")
        if name.endswith("LN fold off"):
            eng.set_ln_fold(False)
        if not fused:
            eng.lib.smtts_test_set_fused_ffn(eng.h, 0)
        yield
    finally:
        eng.set_tuning("latency")
        eng.set_ln_fold(True)
        eng.lib.smtts_test_set_fused_ffn(eng.h, 1)


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Buffers:
    """The device buffers of one test: every input, output and the workspace keeps its address from run to run; inputs are copied in,
    outputs and the workspace are zero-filled before every run."""

    def __init__(self, eng):
        self.eng, self.t = eng, {}

    def _get(self, name, shape, dtype):
        t = self.t.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = self.t[name] = torch.zeros(tuple(shape), dtype=dtype, device=self.eng.device)
        return t

    def inp(self, name, src, dtype=None):
        t = self._get("in:" + name, src.shape, dtype or src.dtype)
        t.copy_(src.to(t.dtype))
        return t

    def out(self, name, shape, dtype=F32):
        return self._get("out:" + name, shape, dtype).zero_()

    def ws(self, nbytes):
        t = self._get("ws", (max(int(nbytes), 1),), U8).zero_()
        assert t.data_ptr() % 256 == 0
        return t

    def call(self, what, rc):
        torch.cuda.synchronize()
        assert rc == 0, f"{what}: rc {rc}: {self.eng.lib.smtts_last_error(self.eng.h).decode()}"


# ---- the entries: inputs (host or device tensors) -> clones of the results ---------------------------------------------------------
def run_cond(eng, buf, i):
    B, R, _ = i["ref"].shape
    P = i["ids"].shape[1]
    ref, rl, ids, pm = buf.inp("ref", i["ref"]), buf.inp("ref_len", i["ref_len"], I64), buf.inp("ids", i["ids"], I64), buf.inp("ph_mask", i["ph_mask"])
    o = dict(k_ref=buf.out("k_ref", (12, B, 8, R, 120)), v_ref=buf.out("v_ref", (12, B, 8, R, 120)), ref_mask=buf.out("ref_mask", (B, R), BOOL),
             k_text=buf.out("k_text", (12, B, 8, P, 120)), v_text=buf.out("v_text", (12, B, 8, P, 120)), ref_seq=buf.out("ref_seq", (B, R, 960)),
             phoneme_mem=buf.out("phoneme_mem", (B, P, 960)))
    ws = buf.ws(eng.lib.smtts_cond_workspace_bytes(eng.h, B, R, P))
    buf.call("smtts_cond_encode", eng.lib.smtts_cond_encode(eng.h, eng._stream(), p(ref), p(rl), p(ids), p(pm), B, R, P, p(o["k_ref"]), p(o["v_ref"]),
                                                            p(o["ref_mask"]), p(o["k_text"]), p(o["v_text"]), p(ws), ws.numel(), p(o["ref_seq"]),
                                                            p(o["phoneme_mem"])))
    return {k: v.clone() for k, v in o.items()}


def _cache_in(buf, i, cache):
    g = {n: buf.inp(n, cache[n]) for n in PC.CACHE_TENSORS}
    g["ref_mask"], g["ph_mask"] = buf.inp("ref_mask", i["ref_mask"]), buf.inp("ph_mask", i["ph_mask"])
    return g


def run_denoise(eng, buf, i, cache):
    B, N, _ = i["x_t"].shape
    R, P = cache["k_ref"].shape[3], cache["k_text"].shape[3]
    x, m, t, g = buf.inp("x_t", i["x_t"]), buf.inp("mask", i["mask"]), buf.inp("t", i["t"]), _cache_in(buf, i, cache)
    v = buf.out("velocity", (B, N, 64))
    ws = buf.ws(eng.lib.smtts_denoise_workspace_bytes(eng.h, B, N, R, P))
    buf.call("smtts_denoise_step", eng.lib.smtts_denoise_step(eng.h, eng._stream(), p(x), p(m), p(t), p(g["k_ref"]), p(g["v_ref"]), p(g["ref_mask"]),
                                                              p(g["k_text"]), p(g["v_text"]), p(g["ph_mask"]), None, B, N, R, P, p(v), p(ws), ws.numel()))
    return dict(velocity=v.clone())


def run_sample(eng, buf, i, cache, kind="plain", ode_cfg=False, start_step=0):
    """kind plain / align / pinned.  Mode 0: 4 steps, noise (4, B, N, 64).  ode_cfg: mode 1 with cfg, 3 steps, noise (B, N, 64); mask,
    caches and their masks carry 3 B rows."""
    B, N = i["mask"].shape
    R, P = cache["k_ref"].shape[3], cache["k_text"].shape[3]
    steps = 3 if ode_cfg else 4
    m, g = buf.inp("mask", i["mask3"] if ode_cfg else i["mask"]), _cache_in(buf, i, cache)
    nz = buf.inp("noise", i["noise1"] if ode_cfg else i["noise"])
    assert g["k_ref"].shape[1] == m.shape[0] == (3 * B if ode_cfg else B) and nz.data_ptr() % 16 == 0
    o = dict(x_out=buf.out("x_out", (B, N, 64)), steps_out=buf.out("steps_out", (steps, B, N, 64)))
    if kind != "plain":
        o["text_mass"] = buf.out("text_mass", (B, N, P))
    ws = buf.ws(eng.lib.smtts_sample_workspace_bytes(eng.h, B, N, R, P, steps, int(ode_cfg)))
    head = (eng.h, eng._stream(), int(ode_cfg), steps, int(ode_cfg), 2.0, 1.5, p(m), p(g["k_ref"]), p(g["v_ref"]), p(g["ref_mask"]), p(g["k_text"]),
            p(g["v_text"]), p(g["ph_mask"]), B, N, R, P, p(nz), C.c_uint64(77), p(o["x_out"]), p(o["steps_out"]), p(ws), ws.numel())
    if kind == "plain":
        buf.call("smtts_sample", eng.lib.smtts_sample(*head))
    elif kind == "align":
        buf.call("smtts_sample_align", eng.lib.smtts_sample_align(*head, None, 0xFFF, 0xFF, p(o["text_mass"])))      # the tap on the last step
    else:
        xp, pin = buf.inp("x_pin", i["x_pin"]), buf.inp("pin", i["pin"])
        assert xp.data_ptr() % 16 == 0
        buf.call("smtts_sample_pinned", eng.lib.smtts_sample_pinned(*head, None, 0xFFF, 0xFF, p(o["text_mass"]), p(xp), p(pin), start_step))
    return {k: v.clone() for k, v in o.items()}


def run_codec(eng, buf, i):
    if "latents" in i:
        B, T, _ = i["latents"].shape
        x, y = buf.inp("latents", i["latents"]), buf.out("audio", (B, 1, eng.hop * T))
        ws = buf.ws(eng.lib.smtts_decode_workspace_bytes(eng.h, B, T))
        buf.call("smtts_codec_decode", eng.lib.smtts_codec_decode(eng.h, eng._stream(), p(x), B, T, p(y), p(ws), ws.numel()))
        return dict(audio=y.clone())
    B, _, S = i["audio"].shape
    x, y = buf.inp("audio", i["audio"]), buf.out("latents", (B, S // eng.hop, 64))
    ws = buf.ws(eng.lib.smtts_encode_workspace_bytes(eng.h, B, S))
    buf.call("smtts_codec_encode", eng.lib.smtts_codec_encode(eng.h, eng._stream(), p(x), B, S, p(y), p(ws), ws.numel()))
    return dict(latents=y.clone())


# ---- the comparison -----------------------------------------------------------------------------------------------------------------
def hold(entry, eng, run, classes, vis, zero_outside=(), note=None):
    """run(cls) -> results.  Every class against `zero` on vis, bit for bit; -> the number of elements compared."""
    n, base = 0, None
    for cls in classes:
        eng.saturations(reset=True)
        res = run(cls)
        sat, rep = eng.saturations(reset=True), eng.lib.smtts_range_report(eng.h).decode()
        for name, t in res.items():
            assert bool(torch.isfinite(t.float()).all()), f"{entry}: `{name}` is not finite everywhere with class `{cls}` behind the masks"
        for name in zero_outside:
            out = ~vis[name].to(res[name].device).expand(res[name].shape)
            assert not bool(res[name][out].any()), f"{entry}: `{name}` is not 0 outside its visible part with class `{cls}`"
        if cls == "zero":
            base = (res, sat, rep)
            continue
        for name, t in res.items():
            n += PC.assert_visible_equal(entry, cls, name, t, base[0][name], vis[name], MASS_AXES if name == "text_mass" else "")
        if cls == "draw":
            assert sat == base[1], f"{entry}: another draw behind the masks moves the saturation counters: {sat} against {base[1]}"
            assert rep == base[2], f"{entry}: another draw behind the masks moves the range report: {rep!r} against {base[2]!r}"
        elif note is not None:
            note["large"] = {k: v for k, v in sat.items() if v}
            note["zero"] = {k: v for k, v in base[1].items() if v}
    return n


def sweep(request, entry, eng, make_run, classes, vis, zero_outside=(), settings=SETTINGS, fused=(True,)):
    """make_run() -> run(cls), called inside every setting.  Prints the line of the test id."""
    total, notes = 0, {}
    for s in settings:
        for f in fused:
            tag = s + ("" if f else ", unfused FFN")
            with setting(eng, s, f):
                note = notes.setdefault(tag, {})
                total += hold(f"{entry} [{tag}]", eng, make_run(), classes, vis, zero_outside, note)
    LARGE_CLAMPS[request.node.name] = notes
    clamps = "; ".join(f"{tag}: large {n.get('large')} zero {n.get('zero')}" for tag, n in notes.items() if n.get("large") or n.get("zero"))
    print(f"\n[padding] {request.node.name}: {total} elements bit for bit" + (f"; clamps {clamps}" if clamps else ""))
    assert total > 0
    return total


def dit_setup(golden_seed, shape, preset, row=None, start_step=0, cfg=False):
    """(engine, case, the zero-class caches of the case on the device, their Case for painting, buffers)"""
    eng = engine("dit", preset, golden_seed)
    c = PC.dit_case(shape, row=row, start_step=start_step)
    if cfg:
        c = PC.cfg_case(c)
    i = c.inputs
    cache = eng.cond_encode(i["ref"], i["ref_len"], i["ids"], i["ph_mask"])
    torch.cuda.synchronize()
    return eng, c, PC.cache_case({n: cache[n] for n in PC.CACHE_TENSORS}, i["ref_mask"], i["ph_mask"], row=row), Buffers(eng)


def painted(c, cc, only=None):
    """class -> (inputs, caches) painted, once per test.  only: the names that are painted (the others stay `zero`)."""
    out = {}
    for cls in c.classes:
        z_i, z_c = PC.paint(c, "zero"), PC.paint(cc, "zero")
        p_i, p_c = PC.paint(c, cls), PC.paint(cc, cls)
        if only is not None:
            p_i = {k: (v if k in only else z_i[k]) for k, v in p_i.items()}
            p_c = {k: (v if k in only else z_c[k]) for k, v in p_c.items()}
        out[cls] = (p_i, p_c)
    return out


# ---- padding: the DiT entries ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cond_encode(request, golden_seed, shape, preset):
    eng, c, _, buf = dit_setup(golden_seed, shape, preset)
    ins = {cls: PC.paint(c, cls) for cls in c.classes}
    sweep(request, "smtts_cond_encode", eng, lambda: (lambda cls: run_cond(eng, buf, ins[cls])), c.classes, PC.dit_visible(c.inputs))


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_denoise_step(request, golden_seed, shape, preset):
    eng, c, cc, buf = dit_setup(golden_seed, shape, preset)
    ins = painted(c, cc)
    sweep(request, "smtts_denoise_step", eng, lambda: (lambda cls: run_denoise(eng, buf, *ins[cls])), c.classes, PC.dit_visible(c.inputs))


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_dmd(request, golden_seed, shape, preset):
    eng, c, cc, buf = dit_setup(golden_seed, shape, preset)
    ins = painted(c, cc)
    sweep(request, "smtts_sample (mode 0, 4 steps)", eng, lambda: (lambda cls: run_sample(eng, buf, *ins[cls])), c.classes, PC.dit_visible(c.inputs))


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_ode_cfg(request, golden_seed, shape, preset):
    """Mode 1 with cfg, 3 steps: 3 B rows of masks and caches, the dropped text and the dropped reference hidden as a whole."""
    eng, c, cc, buf = dit_setup(golden_seed, shape, preset, cfg=True)
    ins = painted(c, cc)
    B = c.inputs["mask"].shape[0]
    sweep(request, "smtts_sample (mode 1, cfg, 3 steps)", eng, lambda: (lambda cls: run_sample(eng, buf, *ins[cls], ode_cfg=True)), c.classes,
          PC.dit_visible(c.inputs, batch=B))


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_align(request, golden_seed, shape, preset):
    eng, c, cc, buf = dit_setup(golden_seed, shape, preset)
    ins = painted(c, cc)
    sweep(request, "smtts_sample_align", eng, lambda: (lambda cls: run_sample(eng, buf, *ins[cls], kind="align")), c.classes,
          PC.dit_visible(c.inputs), zero_outside=("text_mass",))


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("start_step", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_sample_pinned(request, golden_seed, shape, start_step, preset):
    """start_step 0: x_pin is hidden wherever pin && mask is false; 1: behind the mask only.  pin bytes are hidden behind the mask."""
    eng, c, cc, buf = dit_setup(golden_seed, shape, preset, start_step=start_step)
    ins = painted(c, cc)
    K = (c.inputs["pin"] & c.inputs["mask"]).to(eng.device)

    def run(cls):
        res = run_sample(eng, buf, *ins[cls], kind="pinned", start_step=start_step)
        assert torch.equal(res["x_out"][K], ins["zero"][0]["x_pin"].to(eng.device)[K]), f"class `{cls}`: a pinned frame moved"
        assert not bool(res["steps_out"][:start_step].any())                 # slots below start_step are not written
        return res
    sweep(request, f"smtts_sample_pinned (start_step {start_step})", eng, lambda: run, c.classes, PC.dit_visible(c.inputs), zero_outside=("text_mass",))


# ---- padding: the codec (no lengths in the ABI: the hidden region is the future) -------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("kind", ["decode", "encode"])
@pytest.mark.parametrize("spec", list(PC.CODEC_SPECS))
def test_codec(request, spec, kind, preset):
    """The liveness control of a causal network: the painted future must be heard behind the cut, in every setting."""
    eng = engine(spec, preset)
    assert eng.hop == 3200
    c, buf = PC.codec_case(kind, eng.hop), Buffers(eng)
    ins = {cls: PC.paint(c, cls) for cls in c.classes}
    vis = PC.codec_visible(c)
    (out, v), = vis.items()
    seen = {}

    def run(cls):
        seen[cls] = run_codec(eng, buf, ins[cls])
        if cls == "draw":
            assert PC.first_difference(seen["draw"][out], seen["zero"][out], ~v) is not None, f"codec {kind}: the painted future changed nothing behind the cut"
        return seen[cls]
    sweep(request, f"smtts_codec_{kind} ({spec})", eng, lambda: run, c.classes, vis, fused=(True, False))


# ---- row isolation: every other row of the batch redrawn, lengths and masks kept --------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("entry", ["cond_encode", "denoise_step", "sample"])
def test_dit_rows_do_not_see_each_other(request, golden_seed, entry, preset):
    total = 0
    for row in range(3):
        eng, c, cc, buf = dit_setup(golden_seed, "small", preset, row=row)
        ins = {cls: (PC.paint(c, cls), PC.paint(cc, cls)) for cls in ("zero", "draw")}
        run = {"cond_encode": lambda cls: run_cond(eng, buf, ins[cls][0]), "denoise_step": lambda cls: run_denoise(eng, buf, *ins[cls]),
               "sample": lambda cls: run_sample(eng, buf, *ins[cls])}[entry]
        for s in SETTINGS:
            with setting(eng, s):
                total += hold(f"smtts_{entry} [{s}], row {row} with every other row redrawn", eng, run, ("zero", "draw"), PC.dit_visible(c.inputs, row=row))
    print(f"\n[padding] {request.node.name}: {total} elements bit for bit")
    assert total > 0


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("kind", ["decode", "encode"])
@pytest.mark.parametrize("spec", list(PC.CODEC_SPECS))
def test_codec_rows_do_not_see_each_other(request, spec, kind, preset):
    eng, total = engine(spec, preset), 0
    for row in range(2):
        c, buf = PC.codec_case(kind, eng.hop, row=row), Buffers(eng)
        ins = {cls: PC.paint(c, cls) for cls in c.classes}
        for s in SETTINGS[:2]:
            for fused in (True, False):
                with setting(eng, s, fused):
                    total += hold(f"smtts_codec_{kind} ({spec}) [{s}{'' if fused else ', unfused FFN'}], row {row} with the other row redrawn", eng,
                                  lambda cls: run_codec(eng, buf, ins[cls]), c.classes, PC.codec_visible(c))
    print(f"\n[padding] {request.node.name}: {total} elements bit for bit")
    assert total > 0


# ---- liveness: one hidden element declared visible, and the same comparison must fail ---------------------------------------------------
def _flip(i, **at):
    """A copy of the inputs with one more element visible per named mask (ref_len: one more frame)."""
    out = dict(i)
    for name, idx in at.items():
        t = i[name].clone()
        if name == "ref_len":
            t[idx] += 1
        else:
            assert not bool(t[idx].any())
            t[idx] = True
        out[name] = t
    return out


LIVENESS = ["cond_encode", "denoise_step: x_t", "denoise_step: caches", "sample", "sample_ode_cfg", "sample_align", "sample_pinned 0", "sample_pinned 1"]


@pytest.mark.parametrize("what", LIVENESS)
def test_liveness_a_hidden_element_declared_visible_changes_the_row(golden_seed, what):
    """Row 1 of the small shape, class `draw` against `zero`, the masks the same in both runs: frame 9 / reference frame 3 / phoneme 4 of
    row 1 (the first behind each length) now counts, so what row 1 showed before MUST differ: the painted tensors reach the kernels."""
    entry = what.split(":")[0].split(" ")[0]
    start = int(what[-1]) if what.startswith("sample_pinned") else 0
    eng, c, cc, buf = dit_setup(golden_seed, "small", "f16", start_step=start, cfg=(entry == "sample_ode_cfg"))
    B = 3
    only = {"cond_encode": ("ref", "ids"), "denoise_step: x_t": ("x_t",), "denoise_step: caches": PC.CACHE_TENSORS, "sample": ("noise",),
            "sample_ode_cfg": ("noise1",), "sample_align": ("noise",), "sample_pinned 0": ("x_pin",), "sample_pinned 1": ("x_pin",)}[what]
    ins = painted(c, cc, only)
    if what in ("cond_encode", "denoise_step: caches"):
        flip = dict(ref_len=1, ref_mask=(1, 3), ph_mask=(1, 4))
    elif what == "sample_pinned 0":
        flip = dict(pin=(1, 5))                  # a visible, unpinned frame: its x_pin was hidden
    elif entry == "sample_ode_cfg":
        flip = dict(mask=(1, 9), mask3=([1, B + 1, 2 * B + 1], [9, 9, 9]))
    else:
        flip = dict(mask=(1, 9))
    run = {"cond_encode": lambda i, k: run_cond(eng, buf, i), "denoise_step": lambda i, k: run_denoise(eng, buf, i, k),
           "sample": lambda i, k: run_sample(eng, buf, i, k), "sample_ode_cfg": lambda i, k: run_sample(eng, buf, i, k, ode_cfg=True),
           "sample_align": lambda i, k: run_sample(eng, buf, i, k, kind="align"),
           "sample_pinned": lambda i, k: run_sample(eng, buf, i, k, kind="pinned", start_step=start)}[entry]
    zero, draw = (run(_flip(ins[cls][0], **flip), ins[cls][1]) for cls in ("zero", "draw"))
    vis = PC.dit_visible(c.inputs, row=1, batch=B)           # what row 1 showed BEFORE the flip
    if what == "sample_pinned 0":
        vis["x_out"] = vis["x_out"].clone()
        vis["x_out"][1, 5] = False
    names = {"cond_encode": ("k_ref", "v_ref", "k_text", "v_text", "ref_seq", "phoneme_mem"), "denoise_step": ("velocity",)}.get(entry, ("x_out",))
    names += ("text_mass",) if entry == "sample_align" else ()
    for name in names:
        assert PC.first_difference(draw[name], zero[name], vis[name]) is not None, f"{what}: `{name}` of row 1 did not notice its new visible element"
    # and with the masks as they were, the same painted tensors change nothing (the control of the control)
    zero, draw = (run(ins[cls][0], ins[cls][1]) for cls in ("zero", "draw"))
    for name in names:
        PC.assert_visible_equal(what, "draw", name, draw[name], zero[name], PC.dit_visible(c.inputs, batch=B)[name], MASS_AXES if name == "text_mass" else "")
