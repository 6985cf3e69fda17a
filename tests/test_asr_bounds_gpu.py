"""GPU: smtts_asr_logprobs, smtts_ctc_score and smtts_ctc_greedy between guard bands (tests/helpers/guarded.py): every buffer of a call
in an allocation of its own with 1 MiB painted either side, the workspace exactly as large as smtts_asr_workspace_bytes says, each
case run with the guards at 0x00 and at 0xFF: guards clean, inputs untouched, the same output bytes.  And every refused argument."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers.guarded import Arena

pytestmark = pytest.mark.gpu
SEED = 3
NC = 198


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def eng():
    from smalltts_amd.engine import HipEngine
    e = HipEngine(0)
    e.load_synthetic(SEED, parts=("asr",))
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


@pytest.mark.parametrize("B,N,lens,skew", [(1, 1, [1], 0), (3, 7, [7, 3, 1], 4), (2, 40, [40, 33], 0), (2, 15, [15, 0], 4)])
def test_all_three_entries_between_guard_bands(eng, B, N, lens, skew):
    g = torch.Generator().manual_seed(N)
    T, P = 4 * N, 5
    a = Arena(eng.device)
    x = a.put("x", torch.randn(B, N, 64, generator=g), skew=skew)
    nl = a.put("n_len", torch.tensor(lens, dtype=torch.int32))
    nb = eng.lib.smtts_asr_workspace_bytes(eng.h, B, N)
    assert nb > 0 and nb % 256 == 0
    ws = a.workspace("ws", nb)
    logp = a.alloc("logp", (B, T, NC), torch.float32, skew=skew)          # skew 4: 4-byte but not 16-byte aligned
    call = lambda: eng.lib.smtts_asr_logprobs(eng.h, eng._stream(), p(x), p(nl), B, N, p(ws), nb, p(logp))
    got = guarded_runs(a, ["logp"], call, "smtts_asr_logprobs", f"{B}x{N} skew {skew}")["logp"]
    want = eng.asr_logprobs(x.clone(), lens)
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()

    b = Arena(eng.device)
    lp = b.put("logp", got.cpu(), skew=skew)
    tl = b.put("t_len", torch.tensor([4 * n for n in lens], dtype=torch.int32))
    tok = b.put("tokens", (3 + torch.arange(P)[None, :] + 10 * torch.arange(B)[:, None]).to(torch.int32))   # distinct: feasible at T = 4
    p0, p1 = b.put("p0", torch.tensor([0] * B, dtype=torch.int32)), b.put("p1", torch.tensor([min(P, 4 * n) for n in lens], dtype=torch.int32))
    nll = b.alloc("nll", (B,), torch.float32, skew=skew)
    ids, n_ids = b.alloc("ids", (B, T), torch.int32, skew=skew), b.alloc("n_ids", (B,), torch.int32)
    call = lambda: eng.lib.smtts_ctc_score(eng.h, eng._stream(), p(lp), p(tl), p(tok), p(p0), p(p1), B, T, P, NC, p(nll))
    s = guarded_runs(b, ["nll"], call, "smtts_ctc_score", f"{B}x{T}x{P}")["nll"].cpu().numpy()
    assert all(np.isfinite(v) if n > 0 else np.isposinf(v) for v, n in zip(s, lens))
    call = lambda: eng.lib.smtts_ctc_greedy(eng.h, eng._stream(), p(lp), p(tl), B, T, NC, p(ids), p(n_ids))
    r = guarded_runs(b, ["ids", "n_ids"], call, "smtts_ctc_greedy", f"{B}x{T}")
    assert all(0 <= int(v) <= 4 * n for v, n in zip(r["n_ids"].cpu(), lens))


def test_refused_arguments_name_the_entry_and_enqueue_nothing(eng):
    from smalltts_amd.engine import HipEngine
    dev = eng.device
    B, N = 2, 5
    x, nl = torch.randn(B, N, 64, device=dev), torch.tensor([5, 3], dtype=torch.int32, device=dev)
    nb = eng.lib.smtts_asr_workspace_bytes(eng.h, B, N)
    ws = torch.zeros(nb + 512, dtype=torch.uint8, device=dev)
    ws = ws[(-ws.data_ptr()) % 256:]
    logp = torch.full((B, 4 * N, NC), -7.0, device=dev)

    def asr(h=eng.h, x=x, nl=nl, B=B, N=N, ws_ptr=ws.data_ptr(), ws_bytes=nb, logp=logp):
        return eng.lib.smtts_asr_logprobs(h, eng._stream(), p(x), p(nl), B, N, C.c_void_p(ws_ptr), ws_bytes, p(logp))

    for kw in (dict(N=226), dict(N=0), dict(B=65), dict(B=0), dict(ws_ptr=ws.data_ptr() + 4), dict(ws_ptr=ws.data_ptr() + 128),
               dict(ws_bytes=nb - 1), dict(ws_ptr=0), dict(x=None), dict(nl=None), dict(logp=None)):
        assert asr(**kw) == 1, kw
        assert b"smtts_asr_logprobs" in eng.lib.smtts_last_error(eng.h), kw
    assert eng.lib.smtts_asr_workspace_bytes(eng.h, 1, 226) == 0 and eng.lib.smtts_asr_workspace_bytes(eng.h, 65, 1) == 0
    assert eng.lib.smtts_asr_workspace_bytes(eng.h, 64, 225) > 0
    bare = HipEngine(0)                                   # no recogniser part: refused with a message; the CTC entries work on it
    assert not bare.has("asr") and eng.has("asr")
    assert asr(h=bare.h) == 1 and b"no recogniser" in bare.lib.smtts_last_error(bare.h)
    with pytest.raises(ValueError, match="recogniser"):
        bare.asr_logprobs(x, [5, 3])
    torch.cuda.synchronize()
    assert bool((logp == -7).all())
    # the Python face: C != 198, a wrong dtype, a strided tensor, another device's shape
    for bad in (torch.empty(B, 4 * N, 197, device=dev), torch.empty(B, 4 * N, NC, device=dev, dtype=torch.float64),
                torch.empty(B, 4 * N, 2 * NC, device=dev)[:, :, ::2], torch.empty(B, 4 * N, NC)):
        with pytest.raises(ValueError, match="out must be"):
            eng.asr_logprobs(x, [5, 3], out=bad)
    with pytest.raises(ValueError):
        eng.asr_logprobs(x.double(), [5, 3])
    with pytest.raises(ValueError):
        eng.asr_logprobs(x, [5])
    good = eng.asr_logprobs(x, [5, 3])
    tok = torch.ones(B, 4, dtype=torch.int32, device=dev)
    nll = torch.full((B,), -7.0, device=dev)
    tab = torch.tensor([[20, 12], [0, 0], [4, 4]], dtype=torch.int32, device=dev)

    def score(lp=good, tok=tok, B=B, T=4 * N, P=4, Cn=NC, nll=nll):
        return bare.lib.smtts_ctc_score(bare.h, bare._stream(), p(lp), p(tab[0]), p(tok), p(tab[1]), p(tab[2]), B, T, P, Cn, p(nll))

    for kw in (dict(B=0), dict(T=0), dict(P=0), dict(P=199), dict(Cn=1), dict(Cn=257), dict(lp=None), dict(tok=None), dict(nll=None)):
        assert score(**kw) == 1 and b"smtts_ctc_score" in bare.lib.smtts_last_error(bare.h), kw
    ids, n_ids = torch.full((B, 4 * N), -7, dtype=torch.int32, device=dev), torch.full((B,), -7, dtype=torch.int32, device=dev)

    def greedy(lp=good, B=B, T=4 * N, Cn=NC, ids=ids, n_ids=n_ids):
        return bare.lib.smtts_ctc_greedy(bare.h, bare._stream(), p(lp), p(tab[0]), B, T, Cn, p(ids), p(n_ids))

    for kw in (dict(B=0), dict(T=0), dict(T=4097), dict(Cn=0), dict(lp=None), dict(ids=None), dict(n_ids=None)):
        assert greedy(**kw) == 1 and b"smtts_ctc_greedy" in bare.lib.smtts_last_error(bare.h), kw
    torch.cuda.synchronize()
    assert bool((nll == -7).all()) and bool((ids == -7).all()) and bool((n_ids == -7).all())
    assert score() == 0 and greedy() == 0                 # ... and the same buffers with good arguments run, on a handle without weights
    torch.cuda.synchronize()
    assert np.isfinite(nll.cpu().numpy()).all()
    for fn, bad in ((lambda t: bare.ctc_score(t, [20, 12], tok, [0, 0], [4, 4]), good.double()),
                    (lambda t: bare.ctc_greedy(t, [20, 12]), good[:, :, ::2])):
        with pytest.raises(ValueError):
            fn(bad)
    with pytest.raises(ValueError):
        bare.ctc_score(good, [20, 12], tok.long(), [0, 0], [4, 4])
