"""The weight layouts of the latent scorers (smalltts_amd/csrc/scorer_pack.hpp: what finalize_asr and finalize_sv upload), held on the
CPU: tests/host/scorer_pack_check.cpp, built with the host compiler and no HIP, packs index-valued weights w[i] = i, and the result
must equal a restatement of the layout written here.  The shapes are the smallest at which each parameter can go wrong; together they
cover every call shape of the two finalizers.  The BatchNorm fold is held to a float64 evaluation, bit for bit.  The same program,
built with the address and undefined-behaviour sanitizers, runs every case clean."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "scorer_pack_check.cpp")
CXX = os.environ.get("CXX", "c++")

BLOCKS = [  # n_out, i_all, i_use, taps, n_pad
    (128, 64, 64, 1, 128),    # two output blocks
    (70, 64, 64, 1, 128),     # a padded tail (asr.proj: 198 -> 256)
    (64, 128, 128, 1, 64),    # two k blocks
    (64, 64, 64, 3, 64),      # taps (blocks.0, the Res2Net bands)
    (64, 192, 64, 1, 64),     # a column subset (asp.tdnn: 6912 / 2304)
]
COLS = [(8, 12, 0, 12), (8, 12, 5, 4)]   # n_out, i_all, i0, i_use: the whole width; i0 > 0 (asp.tdnn's [m ; s] columns)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scorer_pack") / "scorer_pack_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, SRC, "-o", exe], check=True)

    def run(*args, stdin=""):
        r = subprocess.run([exe, *map(str, args)], input=stdin, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stderr   # (a sanitizer report goes to stderr and ends the program)
        return r.stdout.split()
    return run


def blocks_ref(n_out, i_all, i_use, taps, n_pad):
    """[output block][k block][k % 64][output % 64], k = tap * i_use + channel, outputs zero-padded to n_pad"""
    w = np.arange(n_out * i_all * taps).reshape(n_out, i_all, taps)
    wk = np.zeros((n_pad, taps * i_use), dtype=np.int64)
    wk[:n_out] = w[:, :i_use, :].transpose(0, 2, 1).reshape(n_out, taps * i_use)
    return wk.reshape(n_pad // 64, 64, taps * i_use // 64, 64).transpose(0, 2, 3, 1).ravel()


@pytest.mark.parametrize("case", BLOCKS)
def test_pack_blocks64(check, case):
    want = blocks_ref(*case)
    got = np.array(check("blocks", *case), dtype=np.int64)
    assert got.shape == want.shape and (got == want).all()
    n_out, n_pad = case[0], case[4]
    if n_pad > n_out:   # the padded outputs are zeros, and nothing else is (w[0] = 0 sits at the front)
        assert (got != 0).sum() == n_out * case[2] * case[3] - 1


@pytest.mark.parametrize("case", COLS)
def test_pack_cols(check, case):
    n_out, i_all, i0, i_use = case
    want = np.arange(n_out * i_all).reshape(n_out, i_all)[:, i0:i0 + i_use].T.ravel()
    got = np.array(check("cols", *case), dtype=np.int64)
    assert got.shape == want.shape and (got == want).all()


def _bits(a):
    return "\n".join(f"{v:08x}" for v in np.asarray(a, dtype=np.float32).view(np.uint32)) + "\n"


def test_fold_batchnorm_bits(check):
    rng = np.random.default_rng(5)
    n = 64
    g, be, mu = (rng.uniform(-2, 2, n).astype(np.float32) for _ in range(3))
    var = rng.uniform(0, 3, n).astype(np.float32)
    var[:2] = 0.0   # (the epsilon alone)
    s = g.astype(np.float64) / np.sqrt(var.astype(np.float64) + 1e-5)
    sh = be.astype(np.float64) - mu.astype(np.float64) * s
    # both sides round a double to float once; the program's double may differ from numpy's in the last place (a fused multiply-add
    # in the shift), which cannot change the float unless the double sits next to a rounding boundary of float32: ruled out here
    for d in (s, sh):
        assert (np.nextafter(d, -np.inf).astype(np.float32) == np.nextafter(d, np.inf).astype(np.float32)).all()
    out = check("bn", n, stdin=_bits(g) + _bits(be) + _bits(mu) + _bits(var))
    assert out[0] == "ok"
    got = np.array([int(v, 16) for v in out[1:]], dtype=np.uint32)
    want = np.concatenate([s.astype(np.float32), sh.astype(np.float32)]).view(np.uint32)
    assert got.shape == want.shape and (got == want).all()


@pytest.mark.parametrize("bad", [-0.1, float("nan")])
def test_fold_batchnorm_refuses(check, bad):
    one = np.ones(3, dtype=np.float32)
    var = one.copy()
    var[1] = bad
    assert check("bn", 3, stdin=_bits(one) * 3 + _bits(var)) == ["refused"]
