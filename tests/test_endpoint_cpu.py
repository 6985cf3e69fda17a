"""CPU: the endpoint definition (include/smalltts_hip.h smtts_endpoints / smtts_stitch_seg) restated in numpy
(tests/helpers/endpoint_ref.py) against naive loops written from its wording, the host-side plan of a trimmed join, the
Endpointing conversions, the C header / ctypes table and the server's query parsing.  No GPU."""
import http.client
import re
import threading
from concurrent.futures import Future
from http.server import ThreadingHTTPServer

import numpy as np
import pytest

from smalltts_amd import _lib
from smalltts_amd import server as S
from smalltts_amd.api import HOP_SIZE, Endpointing, as_endpointing, fade_table, plan_long, plan_packed
from tests.helpers import endpoint_ref as R
from tests.helpers.longform_ref import STITCH_CASES, stitch_case, stitch_numpy

W = 240


def _extra_rows():
    """The rows the crafted generator does not hold: (name, x, n, params, expected (start, n) or None)."""
    g = np.random.default_rng(99)
    sp = (g.standard_normal(4000) * 0.2).astype(np.float32)
    click = np.zeros(20 * W, np.float32)
    click[2 * W:4 * W] = (g.standard_normal(2 * W) * 0.2).astype(np.float32)       # two frames, nothing else
    both = np.zeros(40 * W, np.float32)
    both[2 * W:4 * W] = (g.standard_normal(2 * W) * 0.2).astype(np.float32)
    both[20 * W:30 * W] = (g.standard_normal(10 * W) * 0.2).astype(np.float32)
    return [
        ("len = 0", np.zeros(1, np.float32), 0, R.params(), (0, 0)),
        ("len < W", np.full(100, 0.3, np.float32), 100, R.params(min_run=1), (0, 100)),
        ("len < W, min_run 3", np.full(100, 0.3, np.float32), 100, R.params(), (0, 0)),
        ("len not a multiple of W", sp, 4000 - 7, R.params(), (0, 4000 - 7)),
        ("all zero", np.zeros(5000, np.float32), 5000, R.params(), (0, 0)),
        ("all speech", sp, 4000, R.params(lead=0, tail=0), (0, 4000)),
        ("click alone, min_run 3", click, 20 * W, R.params(), (0, 0)),
        ("click alone, min_run 1", click, 20 * W, R.params(min_run=1, lead=0, tail=0), (2 * W, 2 * W)),
        ("click then burst, min_run 3", both, 40 * W, R.params(lead=W, tail=W), (19 * W, 12 * W)),
        ("click then burst, min_run 1", both, 40 * W, R.params(min_run=1, lead=W, tail=W), (W, 30 * W)),
        ("lead / tail larger than the row", both, 40 * W, R.params(lead=10 ** 6, tail=10 ** 6), (0, 40 * W)),
        ("levelled", sp, 4000, R.params(target_rms=np.float32(0.1)), None),
        ("max_gain clamps", sp * np.float32(1e-3), 4000, R.params(target_rms=np.float32(0.1)), None),
        ("peak clamps", sp, 4000, R.params(target_rms=np.float32(0.5)), None),
    ]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_vectorised_reference_equals_the_naive_loops(dt):
    """Energies: the definition fixes no summation order, so the vectorised (pairwise) and the naive (ascending) sums agree to the
    bound of a W-term sum of rounded products and one division, 2 W eps, and exactly where the energy is 0; peaks exactly.  From
    the SAME energies the two decision routines (local window test / sequential run scan) agree exactly, the gain included up to
    its own sum (F + 4) eps."""
    eps = float(np.finfo(dt).eps) / 2
    rows = [(f"seed {s} kind {k}", x, n, R.params(), None) for s in (0, 1, 2) for k, (x, n) in enumerate(R.endpoint_case(s))]
    trimmed = 0
    for name, x, n, p, want in rows + _extra_rows():
        e, pk = R.frame_energy_ref(x, n, W, dt)
        e2, pk2 = R.frame_energy_naive(x, n, W, dt)
        assert e.dtype == e2.dtype == dt and e.shape == e2.shape == ((n + W - 1) // W,), name
        assert np.array_equal(pk, pk2) and np.array_equal(e == 0, e2 == 0), name
        assert (np.abs(e - e2) <= 2 * W * eps * np.abs(e2)).all(), name
        for lvl in (p, dict(p, target_rms=np.float32(0.1))):
            a, b = R.decide_ref(e, pk, n, lvl), R.decide_naive(e, pk, n, lvl)
            assert a[:2] == b[:2], (name, a, b)
            assert abs(float(a[2]) - float(b[2])) <= (len(e) + 4) * eps * float(b[2]), (name, a, b)
        got = R.decide_ref(e, pk, n, p)
        if want is not None:
            assert got[:2] == want and got[2] == 1.0, (name, got)
        trimmed += 0 < got[1] < n
    assert trimmed >= 10


def test_gain_clamps_are_the_stated_ones():
    rows = {name: (x, n, p) for name, x, n, p, _ in _extra_rows()}
    x, n, p = rows["levelled"]
    e, pk = R.frame_energy_ref(x, n, W, np.float64)
    s, m, g = R.decide_ref(e, pk, n, p)
    assert (s, m) == (0, 4000)
    assert abs(g - 0.1 / np.sqrt(np.mean(x.astype(np.float64) ** 2))) < 1e-6 * g      # all frames speech: P is the row's mean power
    x, n, p = rows["max_gain clamps"]
    assert R.endpoints_ref(x, n, p)[2] == float(p["max_gain"])
    x, n, p = rows["peak clamps"]
    g = R.endpoints_ref(x, n, p)[2]
    assert g == float(p["peak_limit"]) / float(np.abs(x).max()) and g < 0.5 / np.sqrt(np.mean(x.astype(np.float64) ** 2))
    assert R.endpoints_ref(np.zeros(5000, np.float32), 5000, R.params(target_rms=np.float32(0.1)))[2] == 1.0


def test_crafted_cases_keep_their_margin_and_decide_alike_in_fp32_and_float64():
    """The condition under which the GPU test may compare the kernel's decisions with the float64 reference: no frame of a crafted
    row lies within 6 dB of its threshold (endpoint_case asserts it), so the two precisions cannot disagree."""
    p = R.params()
    worst, speech, trimmed = np.inf, 0, 0
    for seed in R.CASE_SEEDS:
        for x, n in R.endpoint_case(seed):
            worst = min(worst, R.margin_db(x, n, p))
            a, b = R.endpoints_ref(x, n, p, np.float64), R.endpoints_ref(x, n, p, np.float32)
            assert a[:2] == b[:2]
            speech += a[1] > 0
            trimmed += 0 < a[1] < n
    print(f"smallest margin {worst:.1f} dB, {speech} rows with speech, {trimmed} really trimmed")
    assert worst >= R.MIN_MARGIN_DB and speech >= 80 and trimmed >= 40


@pytest.mark.parametrize("pcm16", [False, True])
@pytest.mark.parametrize("with_gain", [False, True])
def test_stitch_seg_numpy_equals_the_naive_loop(pcm16, with_gain):
    g = np.random.default_rng(5)
    dt = np.int16 if pcm16 else np.float32
    for F in (0, 6, 50):
        audio = (g.standard_normal((5, 1, 96)) * 0.6).astype(np.float32)
        seg = [(1, 37), (0, 0), (33, 63), (7, 1), (0, 96)]            # odd starts, an empty row, F > n / 2, a one-sample row, a whole row
        gain = (g.uniform(0.3, 2.5, 5)).astype(np.float32) if with_gain else None
        offs, S = plan_packed([n for _, n in seg], 0.125)              # 3 samples apart
        fade = fade_table(F / 24.0)
        assert fade.shape == (F,)
        a = R.stitch_seg_numpy(np.zeros(S, dt), audio, seg, gain, offs, fade)
        b = R.stitch_seg_naive(np.zeros(S, dt), audio, seg, gain, offs, fade)
        assert np.array_equal(a, b) and a.any()
    # a window that is the whole row, without gain, is stitch
    for hop, batches, F, gap in STITCH_CASES[:4]:
        rows, fade, S = stitch_case(hop, batches, F, gap, seed=1)
        for audio, lens, offs in rows:
            a = stitch_numpy(np.zeros(S, dt), audio, lens, offs, fade)
            b = R.stitch_seg_numpy(np.zeros(S, dt), audio, [(0, n) for n in lens], None, offs, fade)
            assert np.array_equal(a, b)


def test_plan_packed():
    gap = round(120.0 * 24)
    offs, S = plan_packed([100, 0, 50, 0, 0, 7], 120.0)
    assert offs == [0, 100, 100 + gap, 150 + gap, 150 + gap, 150 + 2 * gap] and S == 157 + 2 * gap   # an empty piece: where the last one ended
    assert plan_packed([0, 0, 9, 0], 120.0) == ([0, 0, 0, 9], 9)      # empty pieces in front and behind: no gap for them
    assert plan_packed([0, 0, 0], 120.0) == ([0, 0, 0], 0) and plan_packed([], 120.0) == ([], 0)
    ns = [7, 16, 11, 5, 9]
    for gap_ms in (0.0, 50.0, 120.0):                                   # nothing trimmed: plan_long's plan
        _, offsets, S = plan_long(ns, 8, gap_ms)
        assert plan_packed([HOP_SIZE * n for n in ns], gap_ms) == (offsets, S)
    with pytest.raises(ValueError):
        plan_packed([3, -1], 0.0)


def test_endpointing_conversions():
    ep = Endpointing()
    p = ep.kernel_params()
    assert p["W"] == 240 and p["min_run"] == 3 and p["lead"] == 720 and p["tail"] == 1440
    for k in ("rel_pow", "floor_pow", "target_rms", "peak_limit", "max_gain"):
        assert isinstance(p[k], np.float32), k
    assert p["rel_pow"] == np.float32(1e-4) and p["floor_pow"] == np.float32(1e-8) and p["target_rms"] == 0.0
    assert p["peak_limit"] == np.float32(10.0 ** (-1 / 20)) and p["max_gain"] == np.float32(10.0)
    q = Endpointing(frame_ms=12.6, rel_db=3, floor_dbfs=-200, min_run=1, lead_ms=0, tail_ms=2.5, level_dbfs=-20, max_gain_db=6).kernel_params()
    assert q["W"] == 4 * round(12.6 * 24 / 4) == 304 and q["lead"] == 0 and q["tail"] == 60 and q["min_run"] == 1
    assert q["rel_pow"] == np.float32(10.0 ** -0.3) and q["floor_pow"] == np.float32(1e-20) and q["target_rms"] == np.float32(0.1)
    assert q["max_gain"] == np.float32(10.0 ** 0.3)
    with pytest.raises(AttributeError):
        ep.min_run = 2
    assert ep == Endpointing() and hash(ep) == hash(Endpointing()) and ep != Endpointing(level_dbfs=-20) and "min_run=3" in repr(ep)
    assert as_endpointing(None) is None and as_endpointing(False) is None and as_endpointing(True) == ep and as_endpointing(ep) is ep
    for bad in (dict(min_run=0), dict(min_run=17), dict(frame_ms=0.1), dict(frame_ms=500), dict(lead_ms=-1), dict(rel_db=float("nan"))):
        with pytest.raises(ValueError):
            Endpointing(**bad)
    with pytest.raises(TypeError):
        as_endpointing("yes")


def test_header_declares_the_endpoint_entries():
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    for name, nargs in (("smtts_endpoints", 19), ("smtts_stitch_seg", 13)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is _lib.i32 and _lib.SIGNATURES[name][1][0] is _lib.vp
    assert _lib.ABI_VERSION >= 10 and re.search(r"#define\s+SMTTS_ABI_VERSION\s+(\d+)", txt).group(1) == str(_lib.ABI_VERSION)


# ---- the server's query parameters, against a stand-in batcher (tests/test_server_cpu.py's manner) --------------------------------
class FakeBatcher:
    def __init__(self):
        self.stats = {"requests": 0}
        self.seen = []

    def submit(self, req):
        self.seen.append(req)
        f = Future()
        y = np.linspace(-1.2, 1.2, S.HOP * S.frames_for(req.duration), dtype=np.float32)
        f.set_result(y if req.trim is None else (y[100:1100] * (np.float32(0.5) if req.trim.level_dbfs is not None else 1), 100))
        return f


@pytest.fixture()
def srv():
    b = FakeBatcher()
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), S.make_handler(b, tokenizer="chars"))
    threading.Thread(target=httpd.serve_forever, kwargs={"poll_interval": 0.02}, daemon=True).start()
    yield httpd.server_address[1], b
    httpd.shutdown()
    httpd.server_close()


def _post(port, query):
    wav = S.encode_wav(np.zeros(4000, np.float32))
    boundary = "----smtts"
    body = b""
    for name, data in (("audio", wav), ("tokens", b"1,2,3")):
        body += f"--{boundary}\r\nContent-Disposition: form-data; name=\"{name}\"\r\n\r\n".encode() + data + b"\r\n"
    body += f"--{boundary}--\r\n".encode()
    c = http.client.HTTPConnection("127.0.0.1", port, timeout=10)
    c.request("POST", "/synthesize?" + query, body=body, headers={"content-type": f"multipart/form-data; boundary={boundary}"})
    r = c.getresponse()
    data = r.read()
    c.close()
    return r.status, {k.lower(): v for k, v in r.getheaders()}, data


def test_parse_trim_query():
    assert S.parse_trim_query({}) is None and S.parse_trim_query({"trim": ["0"]}) is None and S.parse_trim_query({"trim": ["false"]}) is None
    assert S.parse_trim_query({"trim": ["1"]}) == Endpointing() and S.parse_trim_query({"trim": ["true"]}) == Endpointing()
    assert S.parse_trim_query({"trim": ["1"], "level": ["-23.5"]}) == Endpointing(level_dbfs=-23.5)
    for bad in ({"trim": ["2"]}, {"trim": ["yes please"]}, {"level": ["-20"]}, {"trim": ["0"], "level": ["-20"]},
                {"trim": ["1"], "level": ["loud"]}, {"trim": ["1"], "level": ["3"]}, {"trim": ["1"], "level": ["nan"]},
                {"trim": ["1"], "level": ["-100"]}):
        with pytest.raises(S.HttpError) as ei:
            S.parse_trim_query(bad)
        assert ei.value.code == 400, bad


def test_server_trim_query(srv):
    port, b = srv
    st, h0, plain = _post(port, "duration=0.5&seed=1")
    st0, h1, off = _post(port, "duration=0.5&seed=1&trim=0")
    assert st == st0 == 200 and plain == off and "x-smtts-start" not in h0 and "x-smtts-samples" not in h1
    assert b.seen[0].trim is None and b.seen[1].trim is None
    st, h, body = _post(port, "duration=0.5&seed=1&trim=1")
    assert st == 200 and h["x-smtts-start"] == "100" and h["x-smtts-samples"] == "1000" and h["content-type"] == "audio/wav"
    assert len(body) == 44 + 2000 and body[44:] == plain[44 + 200:44 + 2200] and b.seen[2].trim == Endpointing()
    st, h, body = _post(port, "duration=0.5&seed=1&trim=1&level=-20")
    assert st == 200 and h["x-smtts-samples"] == "1000" and b.seen[3].trim == Endpointing(level_dbfs=-20.0)
    n = len(b.seen)
    for bad in ("trim=maybe", "level=-20", "trim=1&level=loud", "trim=1&level=12"):
        st, _, msg = _post(port, "duration=0.5&" + bad)
        assert st == 400 and (b"`trim`" in msg or b"`level`" in msg), (bad, st, msg)
    assert len(b.seen) == n                                             # a refused request never reaches the batcher
