"""Inputs for the padding and row-isolation tests (tests/test_padding_cpu.py, tests/test_padding_gpu.py).  Plain torch on the CPU.

The property: the visible part of row b of a result depends on row b's visible inputs, on the shapes and on the engine's settings, and
on nothing else: not on what lies behind a mask or a length, not on the other rows of the batch.  At the same shape and settings the
launches are the same, so the comparison is bit for bit.

A Case holds the input tensors of an entry with zeros in every hidden region, and for every input that has one its hidden region as a
bool tensor of the input's shape.  paint() overwrites hidden regions only, with one of three classes of values:
  zero   what every other test of the suite has behind its masks;
  draw   another draw of the distribution of the visible data (ids in [1, vocab); pin bytes all set);
  large  1e3 x a draw for ref, x_t, noise and x_pin; 1e4 x a draw (the magnitude of the attention decoys of
         tests/test_attention_edges_gpu.py) for cache tensors handed to an entry; ids and pin bytes another pattern.
Every class has a seed stream of its own, so no two classes agree in a region.

What is excluded.  No NaN and no Inf: the reference itself passes a NaN from a hidden key to every visible row, as 0 x NaN in P V of
its SDPA, so invariance to non-finite hidden values is not a property of the model.  Every id stays in range, every tensor keeps its
full size: no case can fault.  The codec entries take `zero` and `draw` only: a loud tail may trip the f16 FFN range guard, which is
engine state.

Row isolation (row=b): the hidden region is row b's own padding plus EVERY element of every other row; lengths and masks stay, so
the shape and every launch stay, and only row b's visible results are compared."""
from dataclasses import dataclass, field
from typing import Dict, Optional

import torch

from smalltts_amd.weights import CodecSpec

VOCAB = 198          # smalltts_amd.weights.PHONEME_VOCAB
CLASSES = ("zero", "draw", "large")
CODEC_CLASSES = ("zero", "draw")
CACHE_TENSORS = ("k_ref", "v_ref", "k_text", "v_text")
LARGE = {"ref": 1e3, "x_t": 1e3, "noise": 1e3, "noise1": 1e3, "x_pin": 1e3, "k_ref": 1e4, "v_ref": 1e4, "k_text": 1e4, "v_text": 1e4}

# (B, N, R, P), frame lengths, reference lengths, text lengths.  small: a full row, an edge that is no multiple of 4, 8 or 16 and a
# one-frame row, M = 39 inside one GEMM tile and one 16-lane pin group.  tiled: M = 150, the hidden rows 115..149 cross the 64- and
# 128-row tile edges (the ragged shape of tests/test_bounds_gpu.py).
DIT_SHAPES = {"small": ((3, 13, 5, 7), (13, 9, 1), (5, 3, 1), (7, 4, 1)),
              "tiled": ((2, 75, 15, 30), (75, 40), (15, 7), (30, 11))}


# hop 3200 both: the tiny spec of tests/test_bounds_gpu.py, and the entry of tests/test_stream_gpu.py's STREAM_SPECS whose 128- and
# 256-channel stages run the fused mixer and FFN kernels ("no_bias_no_scale_final_norm" of tests/test_codec_gpu.py)
CODEC_SPECS = {"tiny6": CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1)),
               "wide": CodecSpec(n_filters=32, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 2, 1, 1, 1, 1, 2), conv_bias=False, ffn_bias=False,
                                 layer_scale=False, final_norm=True)}
CODEC_SEED = 11


@dataclass
class Case:
    name: str
    inputs: Dict[str, torch.Tensor]                       # hidden regions zero
    hidden: Dict[str, torch.Tensor]                       # input name -> bool tensor of the input's shape
    scale: Dict[str, float] = field(default_factory=dict)  # std of the visible data where it is not 1
    row: Optional[int] = None                             # row isolation: the row whose results are compared
    classes: tuple = CLASSES                              # the classes the case may be painted with


def _prefix(lens, n):
    return torch.arange(n)[None, :] < torch.tensor(lens)[:, None]


def _others(shape, row, dim=0):
    """True on every element whose index along `dim` is not `row`."""
    sel = torch.ones(shape[dim], dtype=torch.bool)
    sel[row] = False
    view = [1] * len(shape)
    view[dim] = shape[dim]
    return sel.view(view).expand(shape).clone()


def dit_case(shape: str, row: Optional[int] = None, start_step: int = 0, seed: int = 0) -> Case:
    """ref, ref_len, ids, ph_mask, x_t, mask, t, noise (4 steps), noise1 (the ODE's single draw), x_pin, pin.  The visible pins: every
    other frame of row 0, the first three frames of row 1, nothing in the rows after it.  start_step picks the hidden region of x_pin:
    0 -> wherever pin && mask is false; >= 1 -> behind the mask only (x_pin is the start of every frame)."""
    (B, N, R, P), nl, rl, pl = DIT_SHAPES[shape]
    g = torch.Generator().manual_seed(7000 + 97 * B + N + seed)
    mask, ref_mask, ph_mask = _prefix(nl, N), _prefix(rl, R), _prefix(pl, P)
    pin = torch.zeros(B, N, dtype=torch.bool)
    pin[0, ::2] = True
    pin[1, :3] = True
    pin &= mask
    K = pin & mask
    m3, r3 = mask[:, :, None].expand(B, N, 64), ref_mask[:, :, None].expand(B, R, 64)
    inputs = dict(ref=torch.randn(B, R, 64, generator=g) * r3, ref_len=torch.tensor(rl), ids=torch.randint(1, VOCAB, (B, P), generator=g) * ph_mask,
                  ph_mask=ph_mask, x_t=torch.randn(B, N, 64, generator=g) * m3, mask=mask, ref_mask=ref_mask, t=torch.rand(B, generator=g),
                  noise=torch.randn(4, B, N, 64, generator=g) * m3, noise1=torch.randn(B, N, 64, generator=g) * m3, pin=pin)
    pin_hidden = ~K if start_step == 0 else ~mask
    inputs["x_pin"] = torch.randn(B, N, 64, generator=g) * (~pin_hidden)[:, :, None]
    hidden = dict(ref=~r3, ids=~ph_mask, x_t=~m3, noise=(~m3)[None].expand(4, B, N, 64).clone(), noise1=~m3,
                  x_pin=pin_hidden[:, :, None].expand(B, N, 64).clone(), pin=~mask)
    hidden = {k: v.clone() for k, v in hidden.items()}
    if row is not None:
        for k, v in hidden.items():
            v |= _others(v.shape, row, dim=1 if k == "noise" else 0)
    return Case(f"dit {shape}" + (f" row {row}" if row is not None else ""), inputs, hidden, row=row)


def cfg_case(c: Case) -> Case:
    """The 3 B-row layout of oracle.dit_oracle.cfg_conditions: [cond ; text dropped ; speaker dropped].  Each row group has hidden
    regions of its own: the dropped text and the dropped reference are hidden as a whole."""
    i = c.inputs
    zl, zp = torch.zeros_like(i["ref_len"]), torch.zeros_like(i["ph_mask"])
    ref_mask3 = torch.cat([i["ref_mask"], i["ref_mask"], torch.zeros_like(i["ref_mask"])], 0)
    inputs = dict(i, ref=torch.cat([i["ref"], i["ref"], torch.zeros_like(i["ref"])], 0), ref_len=torch.cat([i["ref_len"], i["ref_len"], zl], 0),
                  ids=torch.cat([i["ids"], torch.zeros_like(i["ids"]), i["ids"]], 0), ph_mask=torch.cat([i["ph_mask"], zp, i["ph_mask"]], 0),
                  ref_mask=ref_mask3, mask3=i["mask"].repeat(3, 1))
    hidden = dict(c.hidden, ref=~ref_mask3[:, :, None].expand(-1, -1, 64).clone(), ids=~inputs["ph_mask"])
    return Case(c.name + " cfg", inputs, hidden, row=c.row)


def cache_case(cache: Dict[str, torch.Tensor], ref_mask: torch.Tensor, ph_mask: torch.Tensor, row: Optional[int] = None) -> Case:
    """The caches an entry is handed, (L, B, H, R | P, dh): hidden behind ref_mask / ph_mask.  The tensors are NOT copied here (paint
    copies) and may live on a device; the std of the visible part is the scale of a draw."""
    inputs, hidden, scale = {}, {}, {}
    for n in CACHE_TENSORS:
        t = cache[n]
        km = (ref_mask if n.endswith("ref") else ph_mask).cpu()
        h = (~km)[None, :, None, :, None].expand(t.shape).clone()
        if row is not None:
            h |= _others(t.shape, row, dim=1)
        vis = t[(~h).to(t.device)]
        inputs[n], hidden[n] = t, h
        scale[n] = float(vis.double().pow(2).mean().sqrt()) if vis.numel() else 1.0
    return Case("caches", inputs, hidden, scale, row)


def codec_case(kind: str, hop: int, row: Optional[int] = None, seed: int = 0) -> Case:
    """decode: latents (2, 9, 64), rows cut at L = (9, 4): the future latents[b, L[b]:] is hidden, audio[b, :hop L[b]] visible.
    encode: audio (2, 1, 5 hop) at 0.3, L = (5, 2): audio[b, hop L[b]:] is hidden, latents[b, :L[b]] visible."""
    g = torch.Generator().manual_seed(8000 + seed)
    if kind == "decode":
        L, T = (9, 4), 9
        vis = _prefix(L, T)[:, :, None].expand(2, T, 64)
        inputs, hidden, scale = dict(latents=torch.randn(2, T, 64, generator=g) * vis), dict(latents=~vis), {}
    else:
        L, T = (5, 2), 5
        vis = _prefix([hop * n for n in L], hop * T)[:, None, :]
        inputs, hidden, scale = dict(audio=torch.randn(2, 1, hop * T, generator=g) * 0.3 * vis), dict(audio=~vis), dict(audio=0.3)
    hidden = {k: v.clone() for k, v in hidden.items()}
    if row is not None:
        for v in hidden.values():
            v |= _others(v.shape, row)
    c = Case(f"codec {kind}" + (f" row {row}" if row is not None else ""), inputs, hidden, scale, row)
    c.L, c.hop, c.classes = L, hop, CODEC_CLASSES
    return c


def _class_seed(cls: str, seed: int, name: str) -> int:
    return 1_000_003 * (CLASSES.index(cls) + 1) + 7919 * seed + sum(name.encode())


def paint(case: Case, cls: str, seed: int = 0) -> Dict[str, torch.Tensor]:
    """A copy of case.inputs with the hidden regions, and nothing else, overwritten by values of class `cls`.  Tensors without a hidden
    region are passed on as they are.  Values are drawn on the CPU and land on the tensor's own device."""
    assert cls in case.classes, f"{case.name}: class {cls!r} is not one of {case.classes}"
    out = dict(case.inputs)
    for name, h in case.hidden.items():
        if name not in case.inputs:
            continue
        t = case.inputs[name].clone()
        g = torch.Generator().manual_seed(_class_seed(cls, seed, name))
        if cls == "zero":
            v = torch.zeros(t.shape, dtype=t.dtype)
        elif t.dtype == torch.bool:          # pin bytes: all set; then every other one
            v = torch.ones(t.shape, dtype=torch.bool) if cls == "draw" else (torch.arange(t.numel()).view(t.shape) % 2 == 0)
        elif not t.dtype.is_floating_point:  # ids
            v = torch.randint(1, VOCAB, t.shape, generator=g).to(t.dtype)
        else:
            v = torch.randn(t.shape, generator=g) * (case.scale.get(name, 1.0) * (LARGE[name] if cls == "large" else 1.0))
            v = v.to(t.dtype)
        hd = h.to(t.device)
        t[hd] = v.to(t.device)[hd]
        out[name] = t
    return out


# ---- the visible part of every result ----------------------------------------------------------------------------------------------
def _rows(vis: torch.Tensor, row: Optional[int], dim: int = 0) -> torch.Tensor:
    return vis if row is None else vis & ~_others(vis.shape, row, dim)


def dit_visible(inputs: Dict[str, torch.Tensor], row: Optional[int] = None, batch: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """result name -> bool tensor that broadcasts to the result (visible_of expands it).  batch: B of the results of a cfg call, whose
    masks carry 3 B rows (x_out, steps_out and text_mass belong to the B conditional rows)."""
    mask, rm, pm = inputs["mask"], inputs["ref_mask"], inputs["ph_mask"]
    B = batch or mask.shape[0]
    m, p = mask[:B], pm[:B]
    return dict(k_ref=_rows(rm[None, :, None, :, None], row, 1), v_ref=_rows(rm[None, :, None, :, None], row, 1),
                k_text=_rows(pm[None, :, None, :, None], row, 1), v_text=_rows(pm[None, :, None, :, None], row, 1),
                ref_mask=_rows(torch.ones_like(rm), row), ref_seq=_rows(rm[:, :, None], row), phoneme_mem=_rows(pm[:, :, None], row),
                velocity=_rows(m[:, :, None], row), x_out=_rows(m[:, :, None], row), steps_out=_rows(m[None, :, :, None], row, 1),
                text_mass=_rows(m[:, :, None] & p[:, None, :], row))


def codec_visible(case: Case) -> Dict[str, torch.Tensor]:
    hop, L = case.hop, case.L
    if "latents" in case.inputs:
        T = case.inputs["latents"].shape[1]
        return dict(audio=_rows(_prefix([hop * n for n in L], hop * T)[:, None, :], case.row))
    T = case.inputs["audio"].shape[2] // hop
    return dict(latents=_rows(_prefix(L, T)[:, :, None], case.row))


def first_difference(a: torch.Tensor, b: torch.Tensor, vis: torch.Tensor):
    """None where a and b hold the same bits on `vis` (broadcast to their shape), else (index tuple, a's value, b's value) of the first
    element that differs.  NaNs compare by their bits."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    vis = vis.to(a.device).expand(a.shape)
    ia = a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a
    ib = b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b
    bad = (ia != ib) & vis
    if not bool(bad.any()):
        return None
    idx = tuple(int(v) for v in bad.nonzero()[0])
    return idx, a[idx].item(), b[idx].item()


AXES = {5: "(layer, row, head, key, channel)", 4: "(step, row, frame, channel)", 3: "(row, frame, channel)", 2: "(row, key)"}


def assert_visible_equal(entry: str, cls: str, name: str, got: torch.Tensor, want: torch.Tensor, vis: torch.Tensor, axes: str = "") -> int:
    """`got` (hidden values of class cls) holds the bits of `want` (class zero) wherever vis is set; -> the number of elements compared"""
    d = first_difference(got, want, vis)
    assert d is None, (f"{entry}: class `{cls}` behind the masks changes the visible part of `{name}`: first at {axes or AXES.get(got.dim(), 'index')} = "
                       f"{d[0]}: {d[1]!r} with `{cls}`, {d[2]!r} with `zero`")
    return int(vis.expand(got.shape).sum())
