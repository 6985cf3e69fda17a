"""GPU: smtts_sv_embed and smtts_sv_cosine between guard bands (tests/helpers/guarded.py): every buffer of a call in an allocation of
its own with 1 MiB painted either side, the workspace exactly as large as smtts_sv_workspace_bytes says, each case run with the guards
at 0x00 and at 0xFF: guards clean, inputs untouched, the same output bytes.  And every refused argument."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
SEED = 5
D = 192


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0)
    e.load_synthetic(SEED, parts=("sv",))
    e.finalize()
    return e


def guarded_runs(arena, outs, call, entry, case):
    ins = {n: b.view.clone() for n, b in arena.bufs.items() if b.role == "in"}
    snaps = []
    for byte in (0x00, 0xFF):
        arena.paint(byte)
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0, (entry, case, rc)
        arena.assert_clean(entry, f"{case} (guards 0x{byte:02X})")
        snaps.append({n: arena[n].clone() for n in outs})
    for n in outs:
        assert snaps[0][n].cpu().numpy().tobytes() == snaps[1][n].cpu().numpy().tobytes(), (entry, case, n)
    for n, t in ins.items():
        assert arena[n].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), (entry, case, n, "an input changed")
    return snaps[0]


# 65 / 64: either side of sv_tdnn's frame tile; 6 with a row of 0 and of 5 frames: rows without an embedding; 225: the longest row
@pytest.mark.parametrize("B,N,lens,skew", [(1, 6, [6], 0), (3, 7, [7, 6, 3], 4), (2, 70, [65, 64], 0), (3, 15, [15, 0, 5], 4),
                                           (1, 225, [225], 4)])
def test_both_entries_between_guard_bands(eng, B, N, lens, skew):
    g = torch.Generator().manual_seed(N)
    a = Arena(eng.device)
    x = a.put("x", torch.randn(B, N, 64, generator=g), skew=skew)
    nl = a.put("n_len", torch.tensor(lens, dtype=torch.int32))
    nb = eng.lib.smtts_sv_workspace_bytes(eng.h, B, N)
    assert nb > 0 and nb % 256 == 0
    ws = a.workspace("ws", nb)
    emb = a.alloc("emb", (B, D), torch.float32, skew=skew)                # skew 4: 4-byte but not 16-byte aligned
    call = lambda: eng.lib.smtts_sv_embed(eng.h, eng._stream(), p(x), p(nl), B, N, p(ws), nb, p(emb))
    got = guarded_runs(a, ["emb"], call, "smtts_sv_embed", f"{B}x{N} skew {skew}")["emb"]
    want = eng.sv_embed(x.clone(), lens)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    for b, n in enumerate(lens):
        assert bool(got[b].any()) == (n >= 6)

    for K in (1, B):
        c = Arena(eng.device)
        e = c.put("emb", got.cpu(), skew=skew)
        r = c.put("ref", torch.randn(B // K, D, generator=g), skew=skew)
        cos = c.alloc("cos", (B,), torch.float32, skew=skew)
        call = lambda: eng.lib.smtts_sv_cosine(eng.h, eng._stream(), p(e), p(r), B, K, D, p(cos))
        s = guarded_runs(c, ["cos"], call, "smtts_sv_cosine", f"{B} rows K {K}")["cos"].cpu().numpy()
        assert all((abs(v) <= 1.0 and v != 0.0) if n >= 6 else v == 0.0 for v, n in zip(s, lens))


def test_cosine_at_the_odd_widths_between_guard_bands(eng):
    g = torch.Generator().manual_seed(1)
    for B, K, Dn in ((5, 5, 1), (6, 2, 63), (7, 1, 65), (16, 16, 1024)):
        c = Arena(eng.device)
        e, r = c.put("emb", torch.randn(B, Dn, generator=g), skew=4), c.put("ref", torch.randn(B // K, Dn, generator=g))
        cos = c.alloc("cos", (B,), torch.float32, skew=4)
        call = lambda: eng.lib.smtts_sv_cosine(eng.h, eng._stream(), p(e), p(r), B, K, Dn, p(cos))
        s = guarded_runs(c, ["cos"], call, "smtts_sv_cosine", f"{B} rows K {K} D {Dn}")["cos"].cpu().numpy().astype(np.float64)
        a64, r64 = e.cpu().double().numpy(), np.repeat(r.cpu().double().numpy(), K, axis=0)
        want = (a64 * r64).sum(1) / (np.linalg.norm(a64, axis=1) * np.linalg.norm(r64, axis=1))
        assert np.abs(s - want).max() <= (Dn + 8) * 2.0 ** -24


def test_refused_arguments_name_the_entry_and_enqueue_nothing(eng):
    from smalltts_amd.engine import HipEngine
    dev = eng.device
    B, N = 2, 9
    x, nl = torch.randn(B, N, 64, device=dev), torch.tensor([9, 6], dtype=torch.int32, device=dev)
    nb = eng.lib.smtts_sv_workspace_bytes(eng.h, B, N)
    ws = torch.zeros(nb + 512, dtype=torch.uint8, device=dev)
    ws = ws[(-ws.data_ptr()) % 256:]
    emb = torch.full((B, D), -7.0, device=dev)

    def embed(h=eng.h, x=x, nl=nl, B=B, N=N, ws_ptr=ws.data_ptr(), ws_bytes=nb, emb=emb):
        return eng.lib.smtts_sv_embed(h, eng._stream(), p(x), p(nl), B, N, C.c_void_p(ws_ptr), ws_bytes, p(emb))

    for kw in (dict(N=226), dict(N=5), dict(N=0), dict(B=65), dict(B=0), dict(ws_ptr=ws.data_ptr() + 4), dict(ws_ptr=ws.data_ptr() + 128),
               dict(ws_bytes=nb - 1), dict(ws_ptr=0), dict(x=None), dict(nl=None), dict(emb=None)):
        assert embed(**kw) == 1, kw
        assert b"smtts_sv_embed" in eng.lib.smtts_last_error(eng.h), kw
    wsb = eng.lib.smtts_sv_workspace_bytes
    assert wsb(eng.h, 1, 226) == 0 and wsb(eng.h, 65, 6) == 0 and wsb(eng.h, 1, 5) == 0 and wsb(eng.h, 0, 6) == 0
    assert wsb(eng.h, 64, 225) > 0 and wsb(eng.h, 1, 6) > 0
    bare = HipEngine(0)                                   # no verifier part: refused with a message; the cosine works on it
    assert not bare.has("sv") and eng.has("sv")
    assert embed(h=bare.h) == 1 and b"no speaker verifier" in bare.lib.smtts_last_error(bare.h)
    with pytest.raises(ValueError, match="verifier"):
        bare.sv_embed(x, [9, 6])
    torch.cuda.synchronize()
    assert bool((emb == -7).all())
    # the Python face: a wrong width, dtype, a strided tensor, another device; a wrong count of lengths; N under 6
    for bad in (torch.empty(B, 191, device=dev), torch.empty(B, D, device=dev, dtype=torch.float64),
                torch.empty(B, 2 * D, device=dev)[:, ::2], torch.empty(B, D)):
        with pytest.raises(ValueError, match="out must be"):
            eng.sv_embed(x, [9, 6], out=bad)
    for bad_x, ns in ((x.double(), [9, 6]), (x, [9]), (x[:, :5].contiguous(), [5, 5]), (x[:, :, :63], [9, 6])):
        with pytest.raises(ValueError):
            eng.sv_embed(bad_x, ns)
    good = eng.sv_embed(x, [9, 6])
    ref = torch.randn(1, D, device=dev)
    cos = torch.full((B,), -7.0, device=dev)

    def cosine(e=good, r=ref, B=B, K=2, Dn=D, cos=cos):
        return bare.lib.smtts_sv_cosine(bare.h, bare._stream(), p(e), p(r), B, K, Dn, p(cos))

    for kw in (dict(B=0), dict(K=0), dict(K=17), dict(B=3, K=2), dict(Dn=0), dict(Dn=1025), dict(e=None), dict(r=None), dict(cos=None)):
        assert cosine(**kw) == 1 and b"smtts_sv_cosine" in bare.lib.smtts_last_error(bare.h), kw
    torch.cuda.synchronize()
    assert bool((cos == -7).all())
    assert cosine() == 0                                  # ... and the same buffers with good arguments run, on a handle without weights
    torch.cuda.synchronize()
    assert np.isfinite(cos.cpu().numpy()).all()
    for e, r, K in ((good.double(), ref, 2), (good, ref[:, ::2], 2), (good, ref, 1), (good, torch.randn(1, 64, device=dev), 2),
                    (good, ref, 17)):
        with pytest.raises(ValueError):
            bare.sv_cosine(e, r, K)
