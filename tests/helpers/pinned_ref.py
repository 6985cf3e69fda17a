"""The reference of pinned sampling (include/smalltts_hip.h smtts_sample_pinned): the definition's loop around the CPU oracle's
denoise_step, the tiny case the CPU and GPU tests share, and its three oracle runs (computed once per process)."""
import numpy as np
import torch

from oracle import dit_oracle as O


def sample_pinned(w, cache, ph_mask, mask, noise, steps, x_pin=None, pin=None, start=0, keep=None):
    """x = start == 0 ? (K ? x_pin : 0) : x_pin; for i in start .. steps-1: x_t = a x + s noise[i]; v = denoise(x_t, t_i);
    x = K ? x_pin : a x_t - s v.  K = pin & mask.  keep: a list that receives x after every step that ran."""
    b, n = mask.shape
    K = torch.zeros(b, n, 1, dtype=torch.bool) if pin is None else (pin & mask)[:, :, None]
    if start == 0:
        x = torch.zeros(b, n, 64) if x_pin is None else torch.where(K, x_pin, torch.zeros(()))
    else:
        x = x_pin.clone()
    ts = np.linspace(1, 0, steps, dtype=np.float32)
    for i in range(start, steps):
        tv = ts[i]
        a, s = O.alpha_sigma(float(tv))
        x_t = float(a) * x + float(s) * noise[i]
        v = O.denoise_step(w, x_t, mask, torch.full((b,), float(tv)), cache, ph_mask=ph_mask)
        x = float(a) * x_t - float(s) * v
        if x_pin is not None:
            x = torch.where(K, x_pin, x)
        if keep is not None:
            keep.append(x.clone())
    return x


def tiny_case():
    """The tiny case of the issue: B, N, R, P = 2, 12, 5, 7, ragged in row 1, frames [0, 4) and [8, N) of both rows pinned."""
    g = torch.Generator().manual_seed(3)
    B, N, R, P = 2, 12, 5, 7
    ref = torch.randn(B, R, 64, generator=g)
    ids = torch.arange(1, P + 1)[None].repeat(B, 1)
    ph_mask = torch.ones(B, P, dtype=torch.bool)
    ph_mask[1, 5:] = False
    mask = torch.ones(B, N, dtype=torch.bool)
    mask[1, 9:] = False
    noise = torch.randn(4, B, N, 64, generator=g)
    fresh = torch.randn(B, N, 64, generator=g)       # the pinned values of set 2
    pin = torch.zeros(B, N, dtype=torch.bool)
    pin[:, :4] = True
    pin[:, 8:] = True
    return dict(ref=ref, ref_len=torch.tensor([5, 4]), ids=ids, ph_mask=ph_mask, mask=mask, noise=noise, fresh=fresh, pin=pin)


_TINY = {}


def tiny_refs(w):
    """-> (case, cache, plain, set1, set2): the oracle's plain run, the run pinned to the plain run's own result (set 1) and the
    run pinned to fresh normals (set 2), each with its per-step list.  Read-only; computed once."""
    if not _TINY:
        c = tiny_case()
        with torch.no_grad():
            cache = O.encode_conditions(w, c["ref"], c["ref_len"], c["ids"], c["ph_mask"])
            kp, k1, k2 = [], [], []
            plain = sample_pinned(w, cache, c["ph_mask"], c["mask"], c["noise"], 4, keep=kp)
            set1 = sample_pinned(w, cache, c["ph_mask"], c["mask"], c["noise"], 4, plain, c["pin"], keep=k1)
            set2 = sample_pinned(w, cache, c["ph_mask"], c["mask"], c["noise"], 4, c["fresh"], c["pin"], keep=k2)
        _TINY.update(case=c, cache=cache, plain=(plain, kp), set1=(set1, k1), set2=(set2, k2))
    return _TINY["case"], _TINY["cache"], _TINY["plain"], _TINY["set1"], _TINY["set2"]


def free_valid(case):
    """(B, N) bool: the frames that are neither pinned nor behind the mask."""
    return (~case["pin"]) & case["mask"]


def rel(a, b, sel):
    a = np.asarray(a, np.float64)[np.asarray(sel)]
    b = np.asarray(b, np.float64)[np.asarray(sel)]
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
