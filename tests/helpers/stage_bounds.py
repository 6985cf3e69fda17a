"""The rounding arithmetic of the per-stage scorer tests (tests/helpers/sv_stages.py, tests/helpers/asr_stages.py).

A stage's bar is a first-order worst-case bound of the fp32 arithmetic, computed in fp64 from the stage's own inputs, per element:
  * a sum of n terms (a product, a mean, a softmax denominator) may lose n roundings of 2^-24, each relative to the sum of the absolute
    terms: n U sum |term|.  That holds for any summation order (a chain, four segments, a butterfly), so the bar does not know the kernel;
  * an elementwise operation loses one rounding, U |result|;
  * an error that enters an operation leaves it times the operation's Lipschitz constant: ReLU 1, an affine |scale|, a product with
    weights the absolute weights, tanh 1, sigmoid 1/4, SiLU 1.1 (ReLU and the sigmoid by their constant over the interval the
    error allows, relu() and sigmoid_lip() below: 0 for a unit that is dead beyond its error, under 1/4 away from 0), a square root / a division as derived where they stand;
  * a call of a transcendental (or of a composite the kernels write in one expression) loses F ulp of its result, F[name] below,
    and TINY = 2^-126 absolutely where the result can leave fp32's normal range (sigmoid, expf).

F.  The ROCm device-library documentation is not installed next to the compiler this project builds with, so each function was measured
once on an MI355X against double, 2^22 arguments over the range the scorers' taps show (a probe, not a test), at the library's own
compile flags (-O3, no fast-math).  F = twice the worst error seen, at least 2.  Measured, in ulp of the result:
  expf 0.841 on [-80, 0], tanhf 1.333 on [-25, 25], logf 2.308 on [0.5, 400], sqrtf 0.500 on [1e-12, 1e4], 1.0f / x 0.500 on
  [1e-3, 1e4] (both correctly rounded: counted as plain roundings), 1.0f / (1.0f + expf(-v)) 2.623 and v / (1.0f + expf(-v)) 2.559
  on [-30, 30] (both worst near v = -16.68), 1.0f / sqrtf(v) 1.477 on [1e-6, 1e4]   (MI355X, ROCm 7, 2026-10-21).
"""
import torch

U = 2.0 ** -24       # one rounding to nearest, relative
ULP = 2.0 ** -23     # one unit in the last place, relative (at most)
TINY = 2.0 ** -126   # absolute: a result under fp32's smallest normal number may be rounded at 2^-149 or flushed to zero (a saturated
                     # gate of 1e-129, an expf far below the row's maximum); relative bounds say nothing there

# name: (worst ulp error measured, the argument range)
MEASURED = {
    "expf": (0.841, (-80.0, 0.0)),
    "tanhf": (1.333, (-25.0, 25.0)),
    "logf": (2.308, (0.5, 400.0)),
    "sqrtf": (0.5, (1e-12, 1e4)),
    "sigmoid": (2.623, (-30.0, 30.0)),     # 1.0f / (1.0f + expf(-v))
    "silu": (2.559, (-30.0, 30.0)),        # v / (1.0f + expf(-v))
    "rsqrt": (1.477, (1e-6, 1e4)),         # 1.0f / sqrtf(v)
}
F = {k: max(2.0, 2.0 * v[0]) for k, v in MEASURED.items()}
SILU_LIP = 1.1


def bf16(t):
    """t rounded to bfloat16 (8 significant bits), back in t's dtype: the broken operand of the sharpness tests"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def f64(t):
    return torch.as_tensor(t).to(torch.float64)


def dot(a, w, b=None, ea=None, mut=None):
    """a (..., K) times w (O, K) plus b (O) -> (value, error bound); ea: the error bound that a carries.  mut "bf16": both operands
    of the product rounded to bfloat16 (the value only)."""
    K = w.shape[1]
    av, wv = (bf16(a), bf16(w)) if mut == "bf16" else (a, w)
    v = av @ wv.T
    A = a.abs() @ w.abs().T
    n = K
    if b is not None:
        v = v + b
        A = A + b.abs()
        n = K + 1
    e = n * U * A
    if ea is not None:
        e = e + ea @ w.abs().T
    return v, e


def relu(v, ev):
    """ReLU of v with error bound ev -> (value, bound).  Its Lipschitz constant is 1 where the value can be positive and 0 where it
    cannot: max(0, v + d) - max(0, v) = 0 for every |d| <= ev when v + ev < 0 (taken with a margin of 2^-10 ev for what a first-order
    ev leaves out), so a unit that is dead beyond its own error passes none of it on."""
    return torch.relu(v), torch.where(v + ev * (1 + 2.0 ** -10) < 0, torch.zeros_like(ev), ev)


def sigmoid_lip(g, eg):
    """the Lipschitz constant of the sigmoid over [g - eg, g + eg]: s (1 - s) at the point of the interval nearest 0, 1/4 at the most"""
    near = (g.abs() - eg * (1 + 2.0 ** -10)).clamp(min=0)
    s = torch.sigmoid(-near)          # (the small side: 1 - sigmoid(46) is 0.0 in double)
    return s * (1 - s)


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the elements; NaN or inf in got counts as infinite"""
    got, ref, bound = f64(got), f64(ref), f64(bound)
    if not torch.isfinite(got).all():
        return float("inf")
    err = (got - ref).abs()
    r = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    return float(r.max().detach()) if r.numel() else 0.0
