"""CPU: the inputs of the padding tests are fair (tests/helpers/padding_cases.py), before any GPU is involved.

The fp32 oracles have the property exactly: with the hidden regions redrawn (another draw, 1e3 x / 1e4 x a draw) or with every other
row of the batch redrawn, the visible results keep their bits and everything stays finite.  Equality is asserted: a case that showed a
difference here would not be a fair input for the kernels.  The builder itself is checked too: paint touches hidden elements only,
changes every hidden region, keeps ids in range, and its three classes differ."""
import pytest
import torch

from oracle import codec_oracle as CO
from oracle import dit_oracle as O
from oracle.dit_oracle import to_torch
from smalltts_amd.weights import codec_decoder_param_specs, codec_encoder_param_specs, synth_state_dict
from tests.helpers import padding_cases as PC

CODEC_SPECS, CODEC_SEED = PC.CODEC_SPECS, PC.CODEC_SEED
STEPS = 4


# ---- the builder ----------------------------------------------------------------------------------------------------------------------
def _cases():
    out = [PC.dit_case(s, start_step=k) for s in PC.DIT_SHAPES for k in (0, 1)]
    out += [PC.dit_case("small", row=1), PC.cfg_case(PC.dit_case("small"))]
    out += [PC.codec_case(kind, 40, row=row) for kind in ("decode", "encode") for row in (None, 0, 1)]
    g = torch.Generator().manual_seed(1)
    c = PC.dit_case("small")
    cache = {n: torch.randn(12, 3, 8, 5 if n.endswith("ref") else 7, 120, generator=g) * 0.25 for n in PC.CACHE_TENSORS}
    out += [PC.cache_case(cache, c.inputs["ref_mask"], c.inputs["ph_mask"]), PC.cache_case(cache, c.inputs["ref_mask"], c.inputs["ph_mask"], row=2)]
    return out


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.name)
def test_paint_touches_hidden_elements_only_and_all_regions(case):
    painted = {cls: PC.paint(case, cls, seed=3) for cls in case.classes}
    for name, h in case.hidden.items():
        base = case.inputs[name]
        assert h.shape == base.shape and h.dtype == torch.bool and bool(h.any()), name
        for cls, p in painted.items():
            t = p[name]
            assert t is not base and t.dtype == base.dtype
            assert torch.equal(t[~h], base[~h]), f"{case.name}: paint `{cls}` changed a visible element of `{name}`"
            assert bool(torch.isfinite(t.double()).all())
            if not base.dtype.is_floating_point and base.dtype != torch.bool and cls != "zero":      # zero: id 0, as in `ids * ph_mask`
                assert int(t[h].min()) >= 1 and int(t[h].max()) < PC.VOCAB, f"{case.name}: hidden ids of class `{cls}` out of range"
        z, d = painted["zero"][name][h], painted["draw"][name][h]
        assert not bool(z.any()) and bool((d != z).any()), f"{case.name}: classes agree on `{name}`"
        if base.dtype.is_floating_point:
            assert bool((d != 0).all())
        if "large" not in case.classes:                    # the codec entries: a loud tail may trip the range guard, which is engine state
            with pytest.raises(AssertionError):
                PC.paint(case, "large")
            continue
        l = painted["large"][name][h]
        assert bool((l != z).any()) and bool((d != l).any()), f"{case.name}: classes agree on `{name}`"
        if base.dtype.is_floating_point:
            assert bool((l != 0).all())
            want = PC.LARGE[name] if name in PC.LARGE else None
            if want:
                ratio = float(l.double().std() / d.double().std())
                assert 0.5 * want < ratio < 2 * want, (name, ratio)
    for name, t in case.inputs.items():                    # lengths and masks are passed on as they are
        if name not in case.hidden:
            assert all(p[name] is t for p in painted.values()), name


def test_paint_is_a_function_of_class_and_seed():
    c = PC.dit_case("small")
    a, b, other = PC.paint(c, "draw", 1), PC.paint(c, "draw", 1), PC.paint(c, "draw", 2)
    assert all(torch.equal(a[n], b[n]) for n in c.hidden)
    assert all(not torch.equal(a[n], other[n]) for n in c.hidden if n != "pin")


@pytest.mark.parametrize("shape", list(PC.DIT_SHAPES))
def test_pinned_regions_follow_pin_and_mask(shape):
    c0, c1 = PC.dit_case(shape, start_step=0), PC.dit_case(shape, start_step=1)
    mask, pin = c0.inputs["mask"], c0.inputs["pin"]
    K = pin & mask
    assert bool(K.any()) and bool((~K & mask).any())
    assert torch.equal(c0.hidden["x_pin"], (~K)[:, :, None].expand(-1, -1, 64))          # unpinned frames and frames behind the mask
    assert torch.equal(c1.hidden["x_pin"], (~mask)[:, :, None].expand(-1, -1, 64))       # x_pin starts every frame: only the mask hides
    for c in (c0, c1):
        assert torch.equal(c.hidden["pin"], ~mask) and torch.equal(c.inputs["pin"], pin)
        assert not bool(c.inputs["x_pin"][c.hidden["x_pin"]].any()) and bool((c.inputs["x_pin"][~c.hidden["x_pin"]] != 0).all())
    p = PC.paint(c0, "draw")
    assert torch.equal(p["pin"] & mask, K)                                               # K is what it was, whatever lies behind


def test_shapes_and_lengths_are_the_issue_s():
    for (B, N, R, P), nl, rl, pl in PC.DIT_SHAPES.values():
        assert len(nl) == len(rl) == len(pl) == B and max(nl) == N and max(rl) == R and max(pl) == P
        assert min(nl) >= 1 and min(rl) >= 1 and min(pl) >= 1                            # no empty row
    c = PC.dit_case("small", row=1)
    assert bool(c.hidden["ref"][0].all()) and bool(c.hidden["ref"][2].all()) and torch.equal(c.hidden["ref"][1], PC.dit_case("small").hidden["ref"][1])
    assert bool(c.hidden["noise"][:, 0].all()) and not bool(c.hidden["noise"][:, 1, :9].any())
    v = PC.dit_visible(c.inputs, row=1)
    assert not bool(v["velocity"][0].any()) and int(v["velocity"][1].sum()) == 9 and not bool(v["k_ref"][:, 2].any())


# ---- the DiT oracle -------------------------------------------------------------------------------------------------------------------
_zero = {}


def _encode(w, i):
    with torch.no_grad():
        return O.encode_conditions(w, i["ref"], i["ref_len"], i["ids"], i["ph_mask"])


def _with(cache, painted):
    return dict(cache, **{n: painted[n] for n in PC.CACHE_TENSORS})


def _denoise_and_sample(w, i, cache):
    with torch.no_grad():
        v = O.denoise_step(w, i["x_t"], i["mask"], i["t"], cache, ph_mask=i["ph_mask"])
        x = O.sample_dmd(w, cache, i["ph_mask"], i["mask"], i["noise"][:STEPS], STEPS)
    return dict(velocity=v, x_out=x)


def _zero_runs(w, shape):
    """The `zero` runs of a shape: computed once per module and left unchanged."""
    if shape not in _zero:
        c = PC.dit_case(shape)
        i = PC.paint(c, "zero")
        cache = _encode(w, i)
        cc = PC.cache_case(cache, i["ref_mask"], i["ph_mask"])
        _zero[shape] = (c, cache, _denoise_and_sample(w, i, _with(cache, PC.paint(cc, "zero"))))
    return _zero[shape]


COND_OUT = ("k_ref", "v_ref", "k_text", "v_text", "ref_mask", "ref_seq", "phoneme_mem")


def _hold(entry, cls, got, want, vis, names):
    n = 0
    for name in names:
        assert bool(torch.isfinite(got[name].double()).all()), f"{entry}: `{name}` is not finite with class `{cls}`"
        n += PC.assert_visible_equal(entry, cls, name, got[name], want[name], vis[name])
    return n


@pytest.mark.parametrize("shape", list(PC.DIT_SHAPES))
def test_dit_oracle_ignores_what_lies_behind_the_masks(dit_weights, shape):
    c, cache0, res0 = _zero_runs(dit_weights, shape)
    vis = PC.dit_visible(c.inputs)
    n = 0
    for cls in ("draw", "large"):
        i = PC.paint(c, cls)
        assert not torch.equal(i["ref"], c.inputs["ref"]) and not torch.equal(i["ids"], c.inputs["ids"])
        n += _hold("encode_conditions", cls, _encode(dit_weights, i), cache0, vis, COND_OUT)
        cc = PC.cache_case(cache0, i["ref_mask"], i["ph_mask"])        # the caller-owned caches, painted behind their masks
        res = _denoise_and_sample(dit_weights, i, _with(cache0, PC.paint(cc, cls)))
        n += _hold("denoise_step / sample_dmd", cls, res, res0, vis, ("velocity", "x_out"))
    print(f"\n[padding cpu] dit {shape}: {n} elements bit for bit")


def test_cfg_oracle_ignores_what_lies_behind_the_masks(dit_weights):
    """cfg_velocity on the 3 B-row layout: the dropped text and the dropped reference are hidden rows as a whole."""
    c3 = PC.cfg_case(PC.dit_case("small"))
    i = c3.inputs
    cache3 = _encode(dit_weights, i)
    cc = PC.cache_case(cache3, i["ref_mask"], i["ph_mask"])
    vis = PC.dit_visible(i, batch=3)

    def run(cls):
        p, pc = PC.paint(c3, cls), _with(cache3, PC.paint(cc, cls))
        with torch.no_grad():
            return dict(velocity=O.cfg_velocity(dit_weights, p["x_t"], p["mask"], p["t"], pc, p["ph_mask"]))
    want = run("zero")
    for cls in ("draw", "large"):
        _hold("cfg_velocity", cls, run(cls), want, vis, ("velocity",))


@pytest.mark.parametrize("row", [0, 1, 2])
def test_dit_oracle_rows_do_not_see_each_other(dit_weights, row):
    """A row of the small shape (the full one, the ragged one, the one-frame one) with every other row redrawn."""
    c0, cache0, res0 = _zero_runs(dit_weights, "small")
    c = PC.dit_case("small", row=row)
    vis = PC.dit_visible(c.inputs, row=row)
    i = PC.paint(c, "draw")
    other, rl = (row + 1) % 3, int(c.inputs["ref_len"][row])
    assert not torch.equal(i["ref"][other], c.inputs["ref"][other]) and torch.equal(i["ref"][row, :rl], c.inputs["ref"][row, :rl])
    n = _hold(f"encode_conditions, row {row}", "draw", _encode(dit_weights, i), cache0, vis, COND_OUT)
    cc = PC.cache_case(cache0, i["ref_mask"], i["ph_mask"], row=row)
    res = _denoise_and_sample(dit_weights, i, _with(cache0, PC.paint(cc, "draw")))
    n += _hold(f"denoise_step / sample_dmd, row {row}", "draw", res, res0, vis, ("velocity", "x_out"))
    print(f"\n[padding cpu] dit row isolation, row {row}: {n} elements bit for bit")


# ---- the codec oracle -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec_weights():
    return {n: (to_torch(synth_state_dict(codec_decoder_param_specs(s), CODEC_SEED)), to_torch(synth_state_dict(codec_encoder_param_specs(s), CODEC_SEED)))
            for n, s in CODEC_SPECS.items()}


@pytest.mark.parametrize("row", [None, 0, 1])
@pytest.mark.parametrize("kind", ["decode", "encode"])
@pytest.mark.parametrize("spec", list(CODEC_SPECS))
def test_codec_oracle_is_causal_and_row_wise(codec_weights, spec, kind, row):
    """The future of a row (and, with row given, every other row) redrawn: the past keeps its bits."""
    s = CODEC_SPECS[spec]
    assert s.hop == 3200
    c = PC.codec_case(kind, s.hop, row=row)
    w = codec_weights[spec][0 if kind == "decode" else 1]
    out = "audio" if kind == "decode" else "latents"

    def run(cls):
        p = PC.paint(c, cls)
        with torch.no_grad():
            return {out: CO.decode(w, p["latents"], s) if kind == "decode" else CO.encode(w, p["audio"], s)}
    want, got = run("zero"), run("draw")
    _hold(f"codec {kind} ({spec})", "draw", got, want, PC.codec_visible(c), (out,))
    assert not torch.equal(got[out], want[out])            # the painted future is heard behind the cut
