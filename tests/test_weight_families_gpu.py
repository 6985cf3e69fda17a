"""GPU: the DiT and encoder stages held to fp64 under structured weights (tests/helpers/weight_families.py).

Every other stage test runs on weights.init_rule's seeded noise: zero-mean matrices, norm weights near 1, small modulation rows.
Here ONE engine is re-packed (load_state_dict on the changed tensors + finalize) with families that carry the structure of a trained
checkpoint: AdaLN-Zero, a common mode per matrix row, input columns of unequal scale, heavy tails, head-norm weights of both signs
over more than a decade, modulation parts that differ by orders of magnitude; and one input with two massive channels.  These are
synthetic structured weights, not a trained model: nothing here is a claim about speech.

Each output is compared with exact fp64 (oracle/dit_stages.py) as in tests/test_dit_kernels_gpu.py: block increments per utterance
and per row, the emitted image per row, lin / kv outputs per row.  The allowance is BOUND[(kind, preset)] of that file times A(row),
plus its fp32 storage floor for increments.  A = max(1, e_model / e0) comes from the reference alone (the rounding stand-in of
dit_stages under the family against the same stand-in under the synthetic weights; tests/test_weight_families_cpu.py caps it at 8
and shows the near misses): nothing in the allowance is tuned to what the GPU returns under the families.  The zero family is exact:
x_out is x_in bit for bit.  After every case no site has clamped.  Cases run family by family: the stage tensors are loaded first, the
rest before the whole-call check (two finalizes per family).

Found by the clamp check: fold [11, 12) at f16 counted 384 clamps at dit_block with every stored value in range.  The SwiGLU fold
consumer's last column tile (hidden units 2400..2431, computed and dropped) read table entries behind the end of the fold table, the
hook's NaN fill; gemm.hpp LnFoldIn::nh bounds the index now, and that case stays here as the regression test.

Measured on an MI355X (worst error / allowance per family and metric, at bf16x3 | f16 | bf16; records, not bars):
  synth    utt 0.56 | 0.41 | 0.40; row 0.42 | 0.42 | 0.52; image 0.08 | 0.16 | 0.18
  zero     image 0.08 | 0.11 | 0.13; head 0.82 | 0.82 | 0.63
  common   utt 0.43 | 0.49 | 0.38; row 0.30 | 0.42 | 0.47; image 0.08 | 0.33 | 0.22; out 0.41 | 0.48 | -; k 0.40 | 0.46 | -;
           v 0.40 | 0.45 | -; mod 0.36 | 0.36 | 0.66; embed 0.29 | 0.29 | 0.59; head 0.27 | 0.27 | 0.61; velocity 0.09 | - | -
  colscale utt 0.57 | 0.49 | 0.34; row 0.43 | 0.42 | 0.37; image 0.08 | 0.33 | 0.13; out 0.42 | 0.46 | -; k 0.40 | 0.46 | -;
           v 0.41 | 0.45 | -; mod 0.69 | 0.69 | 0.94; embed 0.29 | 0.29 | 0.60; head 0.30 | 0.30 | 0.61; velocity 0.08 | - | -
  heavy    utt 0.55 | 0.47 | 0.35; row 0.39 | 0.43 | 0.34; image 0.08 | 0.35 | 0.13; out 0.40 | 0.47 | -; k 0.40 | 0.46 | -;
           v 0.41 | 0.45 | -; mod 0.49 | 0.49 | 0.93; embed 0.29 | 0.29 | 0.59; head 0.30 | 0.30 | 0.61; velocity 0.08 | - | -
  norms    utt 0.55 | 0.51 | 0.37; row 0.41 | 0.53 | 0.43; image 0.08 | 0.40 | 0.13; out 0.42 | 0.47 | -; k 0.40 | 0.46 | -;
           v 0.39 | 0.45 | -; mod 0.48 | 0.48 | 0.94; embed 0.29 | 0.29 | 0.58; head 0.30 | 0.30 | 0.61; velocity 0.09 | - | -
  mod      utt 0.22 | 0.48 | 0.31; row 0.07 | 0.42 | 0.29; image 0.05 | 0.33 | 0.25; out 0.42 | 0.48 | -; k 0.40 | 0.46 | -;
           v 0.40 | 0.45 | -; mod 0.04 | 0.04 | 0.08; embed 0.29 | 0.29 | 0.58; head 0.30 | 0.30 | 0.61; velocity 0.06 | - | -
"""
import pytest
import torch

from oracle import dit_stages as DS
from tests.helpers import weight_families as WF
from tests.test_dit_gpu import TOL
from tests.test_dit_kernels_gpu import BOUND, _rel_rows

pytestmark = pytest.mark.gpu
ORDER = ("synth",) + WF.FAMILIES
MEASURED = {}    # case id -> (worst error, its allowance, its A)
SEEN = {}        # path -> kernel classes the bounded cases launched
RAN = set()
_ENG = {}


def _engine():
    from smalltts_amd.engine import HipEngine
    if "eng" not in _ENG:
        eng = HipEngine(0)
        eng.load_synthetic(WF.SEED, parts=("dit",))
        eng.finalize()
        _ENG.update(eng=eng, loaded={}, finalizes=0)
    return _ENG["eng"]


def _load(fam, whole=False):
    """the engine under `fam`: the tensors the stage cases read, or all of them (the whole-call check)"""
    eng = _engine()
    base, (f, _) = WF.base_sd(), WF.weights(fam)
    names = list(base) if whole else WF.stage_names(base)
    todo = {}
    for k in names:
        want = fam if WF.changes(fam, k, base[k]) else "synth"
        if _ENG["loaded"].get(k, "synth") != want:
            todo[k] = f[k]
            _ENG["loaded"][k] = want
    if todo:
        eng.load_state_dict(todo)
        eng.finalize()
        _ENG["finalizes"] += 1
    if whole:   # the tensors only the whole call reads are not kept on the host
        keep = set(WF.stage_names(base))
        for k in [k for k in f._made if k not in keep]:
            del f._made[k]
    return eng


def _run(eng, net, what, path="auto", **kw):
    eng.saturations()
    eng.profile(True)
    try:
        res = eng.test_dit_stage(net, what, path=path, **kw)
        torch.cuda.synchronize()
        SEEN.setdefault(path, set()).update(k["name"] for k in eng.profile_report())
    finally:
        eng.profile(False)
    for k, v in res.items():
        assert torch.isfinite(v).all(), f"{net} what={what}: non-finite {k}"
    sat = eng.saturations()
    assert not any(sat.values()), f"{net} what={what}: fp16 producers clamped: {sat}"
    return {k: v.cpu() for k, v in res.items()}


def _hold(cid, errs, allow, A=None):
    """every row / utterance within its own allowance; the record keeps the worst ratio"""
    allow = allow if torch.is_tensor(allow) else torch.full_like(errs, float(allow))
    assert torch.isfinite(errs).all(), f"{cid}: non-finite error"
    i = int((errs / allow).argmax())
    a = float(A[i]) if A is not None else 1.0
    MEASURED[cid] = (float(errs[i]), float(allow[i]), a)
    print(f"[weight families] {cid}: {float(errs[i]):.3e} / {float(allow[i]):.3e} (A {a:.2f})")
    assert errs[i] < allow[i], f"{cid}: {float(errs[i]):.3e} at index {i} (allowance {float(allow[i]):.3e}, A {a:.2f})"


def _hold_all(cid, case, fam, prec, got, ref, bound=None, **kw):
    allow, A = WF.allowance(fam, case, prec, bound)
    errs = case.errors(got, ref, **kw)
    for m in errs:
        _hold(f"{fam} {cid} {prec} {m}", errs[m], allow[m], A[m])


def _blocks(fam, rs, path, l0, l1, prec, massive):
    c = WF.case("blocks", rs, l0, l1, massive)
    eng, w = _load(fam), WF.weights(fam)[1]
    eng.set_precision(prec)
    ref = WF.exact(fam, c)
    res = _run(eng, "dit", 4, path, x=c.x, mask=c.mask, l0=l0, l1=l1, mod=c.table(w), mod_rstride=rs, **c.c)
    img = None
    if path == "fold" and l1 < 12:   # the folded image: (x - c) (1 + scale) of block l1, c the row shift the producers left
        img = (ref["x"] - res["shift"].double()[..., None]) * (1 + DS.block_mod(ref["rows"], l1)[1][:, None])
    _hold_all(f"blocks {path} [{l0},{l1}){' massive' if massive else ''}", c, fam, prec, res, ref, img_ref=img)


def _encoder(fam, net, path, prec):
    eng, w = _load(fam), WF.weights(fam)[1]
    eng.set_precision(prec)
    c = WF.case("enc blocks", net)
    ref = WF.exact(fam, c)
    res = _run(eng, net, 2, path, x=c.x, mask=c.km, l0=0, l1=2)
    img = ref["x"] * w[f"{DS.ENC[net]['prefix']}.2.attention_norm.weight"] if path == "fold" else None   # x times the next norm's weight
    _hold_all(f"{net} blocks {path} [0,2)", c, fam, prec, res, ref, img_ref=img)
    if path != "fold":
        return
    c = WF.case("enc end", net)
    ref = WF.exact(fam, c)
    out = _run(eng, net, 4, x=c.image(w), mask=c.km)["out"]
    assert torch.equal(out[~c.km], torch.zeros_like(out[~c.km])), f"{net} out: rows outside the key mask are not 0"
    kv = _run(eng, net, 8, x=ref["seq"])
    _hold_all(f"{net} out / kv", c, fam, prec, {"out": out, "k": kv["k"], "v": kv["v"]}, ref)


def _cond(fam, prec):
    eng, c = _load(fam), WF.case("cond")
    eng.set_precision(prec)
    got = {"mod": _run(eng, "dit", 1, t=c.t)["mod"], "embed": _run(eng, "dit", 2, x=c.x_t, mask=c.mask)["x"],
           "head": _run(eng, "dit", 8, x=c.img)["out"]}
    _hold_all("mod / embed / head", c, fam, prec, got, WF.exact(fam, c))


def _whole_run(eng, c, tuning):
    eng.saturations()
    prev = eng.set_tuning(tuning)
    try:
        cache = eng.cond_encode(c.ref, c.ref_len, c.ids, c.pm)
        v = eng.denoise_step(c.x_t, c.mask, c.t, cache).cpu()
    finally:
        eng.set_tuning(prev)
    assert torch.isfinite(v[c.mask]).all()
    sat = eng.saturations()
    assert not any(sat.values()), f"whole call: fp16 producers clamped: {sat}"
    return v


def _whole(fam):
    eng, c = _load(fam, whole=True), WF.case("whole")
    eng.set_precision("bf16x3")
    for tuning in ("latency", "throughput"):
        _hold_all(f"cond_encode + denoise_step {tuning}", c, fam, "bf16x3", {"velocity": _whole_run(eng, c, tuning)}, WF.exact(fam, c), bound=TOL)


def _zero_blocks(rs, path, l0, l1, prec):
    """AdaLN-Zero: every gate is 0, a block is the identity bit for bit (masked rows too); the image is LN(x), the head head(LN(x))"""
    c = WF.case("blocks", rs, l0, l1, False)
    eng, w = _load("zero"), WF.weights("zero")[1]
    eng.set_precision(prec)
    table = c.table(w)
    assert not table.any()
    head = l1 == 12
    res = _run(eng, "dit", 4 | (8 if head else 0), path, x=c.x, mask=c.mask, l0=l0, l1=l1, mod=table, mod_rstride=rs, **c.c)
    assert torch.equal(res["x"].view(torch.int32), c.x.view(torch.int32)), f"zero {path} [{l0},{l1}) {prec}: x_out is not x_in bit for bit"
    ln = DS.layer_norm(c.x.double())
    img = c.x.double() - res["shift"].double()[..., None] if path == "fold" and l1 < 12 else ln
    cid = f"zero blocks {path} [{l0},{l1}) {prec}"
    _hold(cid + " image", _rel_rows(res["img"], img), BOUND[("row", prec)])
    if head:
        _hold(cid + " head", _rel_rows(res["out"], DS.head(w, ln)), BOUND[("lin", prec)])


def _zero_cond(prec):
    eng, c = _load("zero"), WF.case("cond")
    eng.set_precision(prec)
    mod = _run(eng, "dit", 1, t=c.t)["mod"]
    assert not mod.any(), f"zero {prec}: the modulation table computed on the GPU is not all +-0"


def _zero_whole():
    eng, c, w = _load("zero", whole=True), WF.case("whole"), WF.weights("zero")[1]
    eng.set_precision("bf16x3")
    with torch.no_grad():
        want = DS.head(w, DS.layer_norm(DS.embed(w, c.x_t.double(), c.mask)))
    for tuning in ("latency", "throughput"):
        v = _whole_run(eng, c, tuning)
        _hold(f"zero cond_encode + denoise_step {tuning} velocity", _rel_rows(v, want)[c.mask.reshape(-1)], BOUND[("lin", "bf16x3")])


def _cases():
    """(family, function, arguments), family by family: the stage cases, then the whole call"""
    out = []
    for fam in ORDER:
        for massive in (True, False):
            if massive and fam not in WF.MASSIVE_FAMILIES or not massive and fam == "synth":
                continue
            for rs, path, precs in WF.BLOCK_RUNS:
                for l0, l1 in WF.BLOCK_RANGES:
                    for p in precs:
                        if fam == "zero":
                            out.append((fam, _zero_blocks, (rs, path, l0, l1, p)))
                        else:
                            out.append((fam, _blocks, (fam, rs, path, l0, l1, p, massive)))
        if fam == "synth":
            continue
        if fam != "zero":
            out += [(fam, _encoder, (fam, net, path, p)) for net in ("style", "text") for path, p in WF.ENC_RUNS]
        out += [(fam, _zero_cond if fam == "zero" else _cond, ((p,) if fam == "zero" else (fam, p))) for p in WF.PRESETS]
        out.append((fam, _zero_whole, ()) if fam == "zero" else (fam, _whole, (fam,)))
    return out


def _id(fam, fn, args):
    return "-".join([fam, fn.__name__.strip("_")] + [str(a) for a in args if a != fam])


@pytest.mark.parametrize("fam,fn,args", [pytest.param(*c, id=_id(*c)) for c in _cases()])
def test_stage_vs_fp64(fam, fn, args):
    fn(*args)
    RAN.add(_id(fam, fn, args))


def test_every_kernel_class_ran_under_the_families():
    """The kernel classes cond_encode, denoise_step (both tunings) and sample (LN-fold) launch at these shapes all ran under a bounded
    case, among them the fold's table kernel, the QKV epilogue and the split-K reduce on the paths that own them (tanh_gates carries no
    profiler name: the `mod` cases read its output); prints the record.  Cases that have not run in this session run here first."""
    for c in _cases():
        if _id(*c) not in RAN:
            c[1](*c[2])
    assert _ENG["finalizes"] <= 2 * len(WF.FAMILIES) + 1, _ENG["finalizes"]
    eng = _load("mod", whole=True)
    g = torch.Generator().manual_seed(10)
    names = set()
    B, N, R, P = WF.BLOCK_SHAPE
    for prec in ("bf16x3", "f16"):   # (the bf16 cases are the fold blocks and mod / embed / head alone)
        eng.set_precision(prec)
        ref, ids = torch.randn(B, R, 64, generator=g), torch.randint(1, 198, (B, P), generator=g)
        pm, mask = torch.ones(B, P, dtype=torch.bool), torch.ones(B, N, dtype=torch.bool)
        eng.profile(True)
        try:
            cache = eng.cond_encode(ref, torch.full((B,), R), ids, pm)
            for tuning in ("latency", "throughput"):
                prev = eng.set_tuning(tuning)
                try:
                    eng.denoise_step(torch.randn(B, N, 64, generator=g), mask, torch.rand(B, generator=g), cache)
                    eng.sample(cache, mask, num_steps=2, noise=torch.randn(2, B, N, 64, generator=g))
                finally:
                    eng.set_tuning(prev)
            torch.cuda.synchronize()
            names.update(k["name"] for k in eng.profile_report())
        finally:
            eng.profile(False)
    print("\n[weight families] worst error / allowance (A) per case:")
    for k, (e, b, a) in sorted(MEASURED.items()):
        print(f"  {k:80s} {e:.3e} / {b:.3e}  ({e / b:.2f}, A {a:.2f})")
    worst = {}
    for k, (e, b, a) in MEASURED.items():
        key = (k.split()[0], k.split()[-1], next((p for p in k.split() if p in WF.PRESETS), ""))
        worst[key] = max(worst.get(key, 0.0), e / b)
    print("[weight families] worst ratio per (family, metric, preset):")
    for k, r in sorted(worst.items()):
        print(f"  {k[0]:9s} {k[1]:9s} {k[2]:7s} {r:.2f}")
    seen = set().union(*SEEN.values())
    assert "fold_vectors" in SEEN["fold"], sorted(SEEN["fold"])
    assert any("qkv_img" in n for n in SEEN["fold"]) and any("qkv_img" in n for n in SEEN["splitk"]) and any("qkv_img" in n for n in SEEN["unsplit"])
    assert any(n.startswith("splitk_resid") for n in SEEN["splitk"]), sorted(SEEN["splitk"])
    skip = {"linspace10", "axpby", "randn", "len_mask"}   # the sampler's own loop and cond_encode's ref_len mask: no stage of the hook
    missing = sorted(n for n in names - seen if n not in skip)
    print("[weight families] product classes:", sorted(names))
    assert not missing, f"kernel classes the product launches that no family case ran: {missing}"
