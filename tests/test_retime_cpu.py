"""CPU: retiming (include/smalltts_hip.h smtts_retime).  The numpy restatement of the kernel's contract
(tests/helpers/retime_ref.py) is held to the algorithm's signal properties: a unit map returns the input's bits, a retimed sine keeps
its pitch and its peak.  The integer maps, the anchor tables and the row cuts of plans.py, the Retime option, the C signature, and
HipEngine.retime against the stand-in library.  And the cases tests/test_retime_gpu.py compares exactly are shown to be clear here:
in every searched segment the best float64 score beats every other candidate's by more than both error bounds."""
import subprocess
import sys

import numpy as np
import pytest

from smalltts_amd import _lib, options, plans
from tests.helpers import retime_ref as R


def _run(c, q_forced=None):
    a = c["anchors"]
    return R.retime_row(c["x"], c["len"], a, len(a), R.window(c["hop"]), c["hop"], c["delta"], int(a[-1, 1]), q_forced=q_forced)


# ---- the algorithm --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop,delta", R.SHAPES)
@pytest.mark.parametrize("name", sorted(R.SIGNALS))
def test_a_unit_map_returns_the_input_bit_for_bit(name, hop, delta):
    n = 50 * hop + 7
    x = R.SIGNALS[name](3, n)
    res = _run(dict(x=x, len=n, anchors=np.asarray([[0, 0], [n, n]]), hop=hop, delta=delta))
    assert res["out_len"] == n and R.searched(res) == 0
    assert res["out"].tobytes() == x.tobytes()
    assert (res["q"] == np.arange(res["K"]) * hop).all()


@pytest.mark.parametrize("speed", R.SPEEDS)
def test_a_retimed_sine_keeps_its_pitch_and_its_peak(speed):
    n, hop, delta = 24000, 240, 120
    x = np.sin(2 * np.pi * 200.0 * np.arange(n) / 24000.0).astype(np.float32)
    anchors, clamped = plans.retime_anchors(n, speed=speed)
    res = _run(dict(x=x, len=n, anchors=anchors, hop=hop, delta=delta))
    y = res["out"]
    assert y.size == int(round(n / speed)) and clamped == []
    rising = int(((y[:-1] < 0) & (y[1:] >= 0)).sum())
    rate = rising / (y.size / 24000.0)
    print(f"speed {speed}: {rate:.2f} rising zero crossings per second, peak {np.abs(y).max():.6f}")
    assert 197.0 <= rate <= 201.0, rate
    assert np.abs(y).max() <= 1.0


def test_the_reference_follows_a_forced_table():
    c = R.uniform_case("voiced", 32, 8, 0.8)
    free = _run(c)
    again = _run(c, q_forced=free["q"])
    assert again["out"].tobytes() == free["out"].tobytes() and (again["q"] == free["q"]).all()
    q = free["q"].copy()
    k = next(k for k, s in enumerate(free["segments"]) if s is not None)
    q[k] += 1 if q[k] + 1 != q[k - 1] + 32 else -1
    forced = _run(c, q_forced=q)
    assert forced["q"][k] == q[k] and forced["out"][:k * 32].tobytes() == free["out"][:k * 32].tobytes()
    assert forced["out"][k * 32:(k + 1) * 32].tobytes() != free["out"][k * 32:(k + 1) * 32].tobytes()


def test_the_tie_rule():
    assert R.pick([-2, -1, 0, 1, 2], np.zeros(5)) == 2                  # the smaller |lag|
    assert R.pick([-2, -1, 1, 2], np.zeros(4)) == 1                     # then the negative lag
    assert R.pick([-2, -1, 0, 1, 2], np.asarray([0, 0, 0, 0, 1e-30])) == 4


# ---- the clear cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.clear_cases()))
def test_the_cases_the_gpu_compares_exactly_are_clear(name):
    res = _run(R.clear_cases()[name])
    print(f"{name}: {res['K']} segments, {R.searched(res)} searched, {R.unclear(res)} unclear")
    assert R.searched(res) >= 10 and R.is_clear(res)


def test_there_are_two_clear_cases_at_each_shape():
    names = sorted(R.clear_cases())
    for hop, delta in R.SHAPES:
        assert sum(n.endswith(f"-{hop}x{delta}") for n in names) >= 2


def test_the_teacher_forced_cases_cover_what_they_are_for():
    cases = R.teacher_cases()
    for hop, delta in R.SHAPES:
        tag = f"{hop}x{delta}"
        for c in (cases[k] for k in cases if k.endswith(tag) or f"-{tag}-" in k):
            assert -(-int(c["anchors"][-1, 1]) // hop) <= 100          # rows of at most 100 segments
        burst = _run(cases[f"burst-{tag}"])
        zero = [s for s in burst["segments"] if s is not None and (s["score"] == 0.0).all() and len(s["lags"]) > 1]
        assert zero and all(s["lags"][s["best"]] == 0 for s in zero)    # exactly-zero scores: the tie rule decides
        assert cases[f"short-{tag}"]["len"] < hop and cases[f"empty-{tag}"]["len"] == 0
        assert int(cases[f"partial-{tag}"]["anchors"][-1, 1]) % hop and int(cases[f"wordlike-{tag}"]["anchors"][-1, 1]) % hop
        a = cases[f"wordlike-{tag}"]["anchors"]
        assert a.shape == (12, 2) and len(set(np.round(np.diff(a[:, 0]) / np.diff(a[:, 1]), 2))) >= 6


# ---- the maps -------------------------------------------------------------------------------------------------------------------
TABLE = np.asarray([[0, 0], [1000, 700], [1500, 1900], [4000, 4400], [4001, 4408], [9000, 6000]], np.int64)


def test_both_maps_are_monotone_and_anchors_map_onto_anchors():
    t = np.arange(0, 6200)
    s = plans.retime_src(t, TABLE)
    assert (np.diff(s) >= 0).all() and (plans.retime_src(TABLE[:, 1], TABLE) == TABLE[:, 0]).all()
    back = plans.retime_times(s, TABLE)
    assert (back <= np.minimum(t, 6000)).all()
    src = np.arange(0, 9100)
    d = plans.retime_times(src, TABLE)
    assert (np.diff(d) >= 0).all() and (plans.retime_times(TABLE[:, 0], TABLE) == TABLE[:, 1]).all()
    assert d[-1] == 6000 and plans.retime_src(6100, TABLE) == 9100 and plans.retime_src(6100, TABLE, n=9000) == 9000
    for v in (0, 1, 699, 700, 1899, 4400, 4407, 5999):
        assert plans.retime_src(v, TABLE) == s[v] and isinstance(plans.retime_src(v, TABLE), int)


def test_the_reference_map_is_the_plan_map_on_a_valid_table():
    M = R.SrcMap(TABLE, len(TABLE), 9000, 9000, 6000)
    ts = list(range(0, 6000, 37))
    assert [M.at(t) for t in ts] == [plans.retime_src(t, TABLE, n=9000) for t in ts]


def test_python_integers_and_int64_agree_near_2_to_the_31():
    big = 2 ** 31 - 1
    table = np.asarray([[0, 0], [big - 5, big // 3], [big, big - 1]], np.int64)
    ts = np.asarray([0, 1, big // 3 - 1, big // 3, big // 3 + 1, big // 2, big - 2], np.int64)
    want = [plans.retime_src(int(t), table) for t in ts]
    assert plans.retime_src(ts, table).tolist() == want
    exact = [int(table[j, 0]) + ((int(t) - int(table[j, 1])) * int(table[j + 1, 0] - table[j, 0])) // int(table[j + 1, 1] - table[j, 1])
             for t, j in zip(ts, [0, 0, 0, 1, 1, 1, 1])]
    assert want == exact
    ss = np.asarray([0, 7, big - 6, big - 5, big - 3, big], np.int64)
    assert plans.retime_times(ss, table).tolist() == [plans.retime_times(int(v), table) for v in ss]


def test_a_table_that_does_not_increase_is_refused():
    for bad in ([[0, 0]], [[0, 1], [5, 5]], [[0, 0], [5, 5], [5, 9]], [[0, 0], [5, 5], [9, 5]], [[-1, 0], [5, 5]]):
        with pytest.raises(ValueError, match="retime_src"):
            plans.retime_src(3, np.asarray(bad))


def test_the_window():
    w = plans.retime_window(240)
    assert w.dtype == np.float32 and w.shape == (480,) and w.tobytes() == R.window(240).tobytes()
    assert np.abs(w[:240].astype(np.float64) + w[240:] - 1.0).max() < 1e-7 and (np.diff(w[:240]) > 0).all()


# ---- retime_anchors -------------------------------------------------------------------------------------------------------------
def _words(spans, kinds=None):
    return [(i, (kinds or {}).get(i, "word"), "x", s, e, -0.1) for i, (s, e) in enumerate(spans)]


def test_uniform_anchor_tables():
    a, c = plans.retime_anchors(24000, speed=1.25)
    assert a.tolist() == [[0, 0], [24000, 19200]] and c == [] and a.dtype == np.int64
    a, c = plans.retime_anchors(24001, duration=30.0)
    assert a.tolist() == [[0, 0], [24001, 720000]]
    for kw in ({}, {"speed": 1.0, "duration": 1.0}, {"speed": 0.0}, {"duration": -1.0}, {"speed": float("nan")},
               {"speed": 1.0, "words": []}, {"to_words": _words([(0, 5)])}):
        with pytest.raises(ValueError, match="retime_anchors"):
            plans.retime_anchors(1000, **kw)


def test_word_targets_land_exactly_and_a_word_outside_the_limits_is_clamped_and_reported():
    now = _words([(1000, 3000), (3000, 3000), (5000, 9000), (12000, 13000), (20000, 24000)], {1: "punct"})
    to = _words([(2000, 4000), (0, 0), (7000, 9500), (11000, 11200), (15000, 20000)], {1: "punct"})
    a, clamped = plans.retime_anchors(30000, words=now, to_words=to)
    assert clamped == [3]                                              # 1000 samples into 200: rate 5 > 2
    assert (np.diff(a, axis=0) > 0).all() and a[0].tolist() == [0, 0] and a[-1, 0] == 30000
    for i, (w, t) in enumerate(zip(now, to)):
        if w[1] != "word":
            continue
        assert plans.retime_times(w[3], a) == t[3]                     # every word keeps its start ...
        if i not in clamped:
            assert plans.retime_times(w[4], a) == t[4]
    assert plans.retime_times(13000, a) == 11000 + 500                 # ... the clamped one at max_rate
    assert a[-1, 1] - a[-2, 1] == a[-1, 0] - a[-2, 0]                  # the tail at speed 1
    rates = np.diff(a[:, 0]) / np.diff(a[:, 1])
    assert rates.min() >= 0.125 and rates.max() <= 8.0
    slow, clamped = plans.retime_anchors(30000, words=now[:1], to_words=_words([(2000, 9000)]))
    assert clamped == [0] and plans.retime_times(3000, slow) == 2000 + 4000       # rate 2/7 < 1/2: the length is clamped
    far, clamped = plans.retime_anchors(30000, words=_words([(16000, 17000)]), to_words=_words([(1000, 2000)]))
    assert clamped == [0] and plans.retime_times(16000, far) == 2000              # a pause at rate 16: moved to rate 8


def test_unequal_word_counts_are_refused():
    now = _words([(0, 5), (9, 12)])
    with pytest.raises(ValueError, match="same word groups"):
        plans.retime_anchors(100, words=now, to_words=now[:1])
    with pytest.raises(ValueError, match="same word groups"):
        plans.retime_anchors(100, words=now, to_words=_words([(0, 5), (9, 12)], {1: "punct"}) + [(2, "word", "x", 20, 30, 0.0)])
    with pytest.raises(ValueError, match="behind"):
        plans.retime_anchors(10, words=now, to_words=now)
    four = [(w[0], w[1], w[3], w[4]) for w in now]                                # synthesize_long's rows
    assert plans.retime_anchors(100, words=four, to_words=four)[0].tolist() == [[0, 0], [5, 5], [9, 9], [12, 12], [100, 100]]


# ---- retime_rows ----------------------------------------------------------------------------------------------------------------
def test_rows_cut_inside_pauses_and_their_maps_concatenate():
    rng = np.random.default_rng(5)
    spans, pos = [], 2000
    for i in range(60):
        n = int(rng.integers(3000, 9000))
        spans.append((pos, pos + n))
        pos += n + (int(rng.integers(5000, 9000)) if i % 4 == 3 else int(rng.integers(0, 3000)))
    n = pos + 1000
    now = _words(spans)
    to = _words([(int(s * 0.8) + 100, int(e * 0.8) + 100) for s, e in spans])
    anchors, clamped = plans.retime_anchors(n, words=now, to_words=to)
    max_row = 60000
    rows, table = plans.retime_rows(n, anchors, now, max_row=max_row)
    assert len(rows) > 4 and {tuple(r) for r in anchors.tolist()} <= {tuple(r) for r in table.tolist()}
    pauses = [(e0, s1) for (_a, e0), (s1, _b) in zip(spans, spans[1:]) if s1 - e0 >= 4800]
    src_pos = dst_pos = 0
    whole = []
    for s0, sn, d0, tab in rows:
        assert (s0, d0) == (src_pos, dst_pos) and tab[0].tolist() == [0, 0] and tab[-1, 0] == sn
        assert 0 < sn <= max_row and 0 < tab[-1, 1] <= max_row
        if s0:
            assert any(e0 < s0 < s1 and s0 == (e0 + s1) // 2 for e0, s1 in pauses), s0     # a cut lies in the middle of a pause
        whole.append(s0 + plans.retime_src(np.arange(int(tab[-1, 1])), tab))
        src_pos, dst_pos = s0 + sn, d0 + int(tab[-1, 1])
    assert (src_pos, dst_pos) == (n, int(anchors[-1, 1]))
    whole = np.concatenate(whole)
    assert (whole == plans.retime_src(np.arange(dst_pos), table)).all()
    assert (plans.retime_times(anchors[:, 0], table) == anchors[:, 1]).all()


def test_rows_without_pauses_cut_at_anchors_and_without_anchors_at_max_row():
    spans = [(i * 5000, i * 5000 + 4000) for i in range(30)]
    now = _words(spans)
    anchors, _c = plans.retime_anchors(150000, words=now, to_words=now)
    rows, table = plans.retime_rows(150000, anchors, now, max_row=24000)
    assert len(table) == len(anchors) and all(r[0] in set(anchors[:, 0].tolist()) for r in rows)
    assert all(r[1] <= 24000 for r in rows)
    uniform, _c = plans.retime_anchors(100000, speed=0.5)
    rows, table = plans.retime_rows(100000, uniform, None, max_row=30000)
    assert all(r[1] <= 30000 and r[3][-1, 1] <= 30000 for r in rows) and sum(int(r[3][-1, 1]) for r in rows) == 200000
    assert [r[3][-1, 1] for r in rows[:-1]] == [30000] * (len(rows) - 1)
    one, table = plans.retime_rows(1000, np.asarray([[0, 0], [1000, 900]]))
    assert len(one) == 1 and one[0][:3] == (0, 1000, 0) and one[0][3].tolist() == [[0, 0], [1000, 900]]


# ---- options and plumbing -------------------------------------------------------------------------------------------------------
def test_the_retime_option():
    r = options.Retime(speed=1.25)
    assert (r.speed, r.duration, r.to_words, r.hop, r.delta, r.min_rate, r.max_rate) == (1.25, None, None, 240, 120, 0.5, 2.0)
    assert options.as_retime(None) is None and options.as_retime(r) is r and options.as_retime(0.8) == options.Retime(speed=0.8)
    assert options.as_retime(2) == options.Retime(speed=2.0) and options.Retime(duration=30).duration == 30.0
    assert options.Retime(to_words=[(0, "word", "x", 0, 5, 0.0)]).to_words == ((0, "word", "x", 0, 5, 0.0),)
    with pytest.raises(AttributeError):
        r.speed = 2.0
    for kw in ({}, {"speed": 1.0, "duration": 2.0}, {"speed": 1.0, "to_words": [(0, "word", 0, 5)]}, {"speed": 0.0}, {"speed": -1.0},
               {"duration": float("inf")}, {"speed": 1.0, "hop": 242}, {"speed": 1.0, "hop": 8}, {"speed": 1.0, "hop": 516},
               {"speed": 1.0, "delta": -1}, {"speed": 1.0, "delta": 513}, {"speed": 1.0, "min_rate": 0.0},
               {"speed": 1.0, "min_rate": 3.0}, {"to_words": []}):
        with pytest.raises(ValueError, match="Retime"):
            options.Retime(**kw)
    for kw in ({"speed": "fast"}, {"speed": True}, {"speed": 1.0, "hop": 240.0}):
        with pytest.raises(TypeError, match="Retime"):
            options.Retime(**kw)
    for bad in (True, "1.0", (1.0, 2.0)):
        with pytest.raises(TypeError, match="retime"):
            options.as_retime(bad)


def test_options_and_plans_still_import_without_torch():
    code = ("import sys\nfrom smalltts_amd.options import Retime, as_retime\nfrom smalltts_amd import plans\n"
            "assert as_retime(1.5).speed == 1.5 and plans.retime_window(16).shape == (32,)\n"
            "assert plans.retime_anchors(100, speed=2.0)[0].tolist() == [[0, 0], [100, 50]]\n"
            "assert 'torch' not in sys.modules and 'smalltts_amd.engine' not in sys.modules\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]


def test_the_entry_is_in_the_signature_table_and_in_the_header():
    assert "smtts_retime" in _lib.SIGNATURES and "smtts_retime" in _lib.header_symbols() and _lib.ABI_VERSION == 11
    res, args = _lib.SIGNATURES["smtts_retime"]
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    decl = txt[txt.index("int smtts_retime("):]
    decl = decl[:decl.index(";")]
    import re
    params = re.sub(r"/\*.*?\*/", "", decl[decl.index("(") + 1: decl.rindex(")")], flags=re.S).split(",")
    assert res is _lib.i32 and len(args) == len(params) == 15
    kinds = [_lib.vp if "*" in p or "smtts_handle" in p else _lib.i64 if "int64_t" in p else _lib.i32 for p in params]
    assert kinds == args


def _engine_call(fn, **opts):
    import smalltts_amd.engine  # noqa: F401  (the stand-in patches the modules that are loaded when it is entered)
    from tests.helpers.engine_cases import operands
    from tests.helpers.engine_standin import record
    return record("retime", fn, operands(), **opts)


GOOD = [np.asarray([[0, 0], [20, 10], [40, 50]]), np.asarray([[0, 0], [24, 30]])]      # for rows of 40 and 24 samples


def test_engine_retime_makes_one_call_with_one_table():
    lines, lib = _engine_call(lambda e, o: e.retime(o.audio, [40, 24], GOOD, hop=16, delta=4, return_q=True))
    assert lib.error is None and [l.split(" ")[0] for l in lines if l.startswith("smtts_")] == ["smtts_retime"]
    call = lines[1].split(" ")
    # h stream audio B row_stride len anchors n_anchor A win hop delta out out_stride q
    assert call[1:6] == ["h", "stream", "audio+0", "2", "64"] and call[6:9] == ["table0+0", "table0+32", "table0+16"]
    assert call[9] == "3" and call[11:13] == ["16", "4"] and call[13:] == ["ret[0]+0", "50", "ret[2]+0"]
    assert lines[2] == "table0 int64(16,) [40, 24, 3, 2, 0, 0, 20, 10, 40, 50, 0, 0, 24, 30, 0, 0]"
    assert lines[-1] == "-> (float32(2, 1, 50), (50, 30), int64(2, 4))"              # (the recorder shows a list as a tuple)
    lines, lib = _engine_call(lambda e, o: (e.retime(o.audio, [40, 24], GOOD), e.retime(o.audio, [40, 24], GOOD)))
    assert lib.error is None and [name for name, _a in lib.calls][:2] == ["smtts_retime"] * 2
    assert lib.calls[0][1][9].tensor is lib.calls[1][1][9].tensor                   # the window is cached
    assert lib.calls[0][1][14] == "null" and lib.calls[0][1][10:12] == ["240", "120"]


@pytest.mark.parametrize("what,anchors,match", [
    ("first dst", [np.asarray([[0, 1], [20, 10]]), GOOD[1]], "start at dst 0"),
    ("src not increasing", [np.asarray([[0, 0], [20, 10], [20, 30]]), GOOD[1]], "increase strictly"),
    ("dst not increasing", [GOOD[0], np.asarray([[0, 0], [10, 30], [24, 30]])], "increase strictly"),
    ("src behind len", [GOOD[0], np.asarray([[0, 0], [25, 30]])], r"must lie in \[0, 24\]"),
    ("src negative", [np.asarray([[-1, 0], [20, 10]]), GOOD[1]], r"must lie in \[0, 40\]"),
    ("slope 9", [np.asarray([[0, 0], [36, 4]]), GOOD[1]], "1/8 to 8 times"),
    ("slope 1/9", [np.asarray([[0, 0], [4, 36]]), GOOD[1]], "1/8 to 8 times"),
    ("one table", [GOOD[0]], "one anchor table per row"),
    ("one anchor", [GOOD[0], np.asarray([[0, 0]])], "integer"),
    ("floats", [GOOD[0], np.asarray([[0.0, 0.0], [24.0, 30.0]])], "integer"),
])
def test_engine_retime_refuses(what, anchors, match):
    lines, lib = _engine_call(lambda e, o: e.retime(o.audio, [40, 24], anchors))
    assert isinstance(lib.error, ValueError) and str(lib.error).startswith("retime: "), (what, lib.error)
    import re
    assert re.search(match, str(lib.error)), (what, lib.error)
    assert not lib.calls, what


def test_engine_retime_refuses_the_rest():
    for fn, match in ((lambda e, o: e.retime(o.audio, [40, 24], GOOD, hop=18), "hop"),
                      (lambda e, o: e.retime(o.audio, [40, 24], GOOD, delta=600), "delta"),
                      (lambda e, o: e.retime(o.audio, [40, 65], GOOD), "lengths"),
                      (lambda e, o: e.retime(o.audio2, [40, 24], GOOD), r"\(B,1,S\)")):
        lines, lib = _engine_call(fn)
        assert isinstance(lib.error, ValueError) and "retime" in str(lib.error) and not lib.calls
        import re
        assert re.search(match, str(lib.error)), lib.error
    lines, lib = _engine_call(lambda e, o: e.retime(o.audio, [40, 24], GOOD), fail=["smtts_retime"])
    assert isinstance(lib.error, RuntimeError) and str(lib.error).startswith("retime: ")


# ---- the layers above the engine, as far as they are host arithmetic -------------------------------------------------------------
def test_the_api_maps_segments_and_words_and_refuses_what_does_not_fit():
    from smalltts_amd import api
    table = np.asarray([[0, 0], [1000, 500], [3000, 3500]])
    assert api._retimed_segments([(0, 1000, 7, 1.0), (1000, 2000, 0, 0.5)], table) == [(0, 500, 7, 1.0), (500, 3000, 0, 0.5)]
    assert api._retimed_words([(0, "word", 200, 1000), (1, "punct", 1000, 1000)], table) == [(0, "word", 100, 500), (1, "punct", 500, 500)]
    assert api._retimed_words([(3, "word", "ab", 2000, 3000, -0.25)], table) == [(3, "word", "ab", 2000, 3500, -0.25)]
    assert api._retimed_words(None, table) is None
    assert api._long_retime("synthesize_long", None, True) is None
    assert api._long_retime("synthesize_long", 1.5, False) == api.Retime(speed=1.5)
    with pytest.raises(ValueError, match=r"synthesize_long: .*SmallTTS\.retime"):
        api._long_retime("synthesize_long", api.Retime(to_words=[(0, "word", "x", 0, 5, 0.0)]), False)
    with pytest.raises(ValueError, match="render_long: .*pcm16"):
        api._long_retime("render_long", api.Retime(duration=2.0), True)
    for name in ("Retime", "as_retime", "retime_anchors", "retime_rows", "retime_times"):
        assert hasattr(api, name)


def test_the_command_lines(tmp_path):
    import json
    from smalltts_amd.scripts import longform
    from smalltts_amd.scripts import retime as cli
    from smalltts_amd.scripts.align import words_json
    rows = [(0, "word", "ab", 0, 800, -0.5), (1, "punct", ",", 800, 800, float("-inf"))]
    p = tmp_path / "w.json"
    p.write_text(words_json(rows), encoding="utf-8")
    assert cli.target_words(str(p)) == rows
    p.write_text(json.dumps({"words": json.loads(words_json(rows)), "speaking_rate": None}), encoding="utf-8")      # align.py --long
    assert cli.target_words(str(p)) == rows
    base = ["--wav", "ref.wav", "--tokens-file", "t.txt", "--durations", "1"]
    assert longform.parse_args(base).retime is None
    assert longform.parse_args(base + ["--speed", "1.25"]).retime == options.Retime(speed=1.25)
    assert longform.parse_args(base + ["--fit-seconds", "30"]).retime == options.Retime(duration=30.0)
    for bad in (["--speed", "1.25", "--fit-seconds", "30"], ["--speed", "0"], ["--speed", "1.1", "--stream"]):
        with pytest.raises(SystemExit):
            longform.parse_args(base + bad)
    for bad in ([], ["--speed", "1", "--duration", "2"]):
        with pytest.raises(SystemExit):
            cli.main(["--wav", "a.wav", "--text", "x", "--out", str(tmp_path / "o.wav")] + bad)
    with pytest.raises(SystemExit):
        cli.main(["--wav", "a.wav", "--speed", "1.1", "--out", str(tmp_path / "o.wav")])                           # no text


# ---- words that abut, a word at sample 0; cuts under pairs at the engine's slope limits ---------------------------------------------
def _landed(now, to, anchors, clamped):
    for w, t in zip(now, to):
        if w[1] == "word" and w[0] not in clamped:
            assert (plans.retime_times(w[3], anchors), plans.retime_times(w[4], anchors)) == (t[3], t[4]), (w, t)


def test_every_word_that_is_not_reported_lands_on_its_target():
    """A word that starts where the anchor in front already sits (it abuts the previous word, or starts at sample 0) cannot be sent
    anywhere else: it is reported, never moved silently."""
    now, to = _words([(1000, 3000), (3000, 5000)]), _words([(1000, 3000), (4000, 6000)])
    a, clamped = plans.retime_anchors(10000, words=now, to_words=to)
    assert clamped == [1] and plans.retime_times(3000, a) == 3000 and plans.retime_times(5000, a) == 5000   # its length is kept
    _landed(now, to, a, clamped)
    now, to = _words([(0, 3000), (3000, 4000), (6000, 6000), (6000, 8000)]), _words([(500, 3500), (3500, 4500), (7000, 7000), (7000, 9500)])
    a, clamped = plans.retime_anchors(10000, words=now, to_words=to)
    assert clamped == [0, 1]                                   # word 1 rides on the word at 0, which cannot start at 500; the pause
    assert plans.retime_times(6000, a) == 7000                 # behind it brings words 2 and 3 back onto their targets
    _landed(now, to, a, clamped)
    now, to = _words([(0, 3000), (3000, 4000), (6000, 8000)]), _words([(0, 2000), (2000, 3500), (5000, 7000)])
    a, clamped = plans.retime_anchors(10000, words=now, to_words=to)
    assert clamped == [] and len(a) == 6                       # abutting words whose targets abut too: nothing moves
    _landed(now, to, a, clamped)
    rng = np.random.default_rng(9)
    for _trial in range(200):                                   # whatever is not reported has landed
        k = int(rng.integers(1, 9))
        cuts = np.sort(rng.integers(0, 40, 2 * k)) * 250
        tcuts = np.sort(rng.integers(0, 40, 2 * k)) * 250
        now, to = _words(list(zip(cuts[::2], cuts[1::2]))), _words(list(zip(tcuts[::2], tcuts[1::2])))
        if all(s == e for _i, _k, _p, s, e, _c in now) and cuts[-1] == 0:
            continue
        a, clamped = plans.retime_anchors(12000, words=now, to_words=to)
        _landed(now, to, a, clamped)
        assert (np.diff(a, axis=0) > 0).all() and (np.diff(a[:, 0]) <= 8 * np.diff(a[:, 1])).all() and (np.diff(a[:, 1]) <= 8 * np.diff(a[:, 0])).all()


def _engine_accepts(tab, n):
    """HipEngine.retime's four checks on one row's table."""
    ds, dd = np.diff(tab[:, 0]), np.diff(tab[:, 1])
    assert tab[0, 1] == 0 and (ds > 0).all() and (dd > 0).all() and tab[0, 0] >= 0 and tab[-1, 0] <= n, tab.tolist()
    assert (ds <= 8 * dd).all() and (dd <= 8 * ds).all(), tab.tolist()


@pytest.mark.parametrize("table,pause", [
    ([[0, 0], [700000, 700000], [716007, 702001], [1400000, 1385994]], (700000, 716007)),       # a pause at rate 8, cut in the middle
    ([[0, 0], [700000, 700000], [702001, 716007], [1385994, 1400000]], (700000, 702001)),       # a pause at rate 1/8
    ([[0, 0], [700000, 700000], [700009, 700002], [1400000, 1399993]], (700000, 700009)),       # 9 source samples onto 2
    ([[0, 0], [700000, 700000], [700002, 700009], [1399993, 1400000]], (700000, 700002)),       # 2 onto 9: no room inside the pair
])
def test_rows_cut_under_a_pair_at_the_slope_limit_pass_the_engines_checks(table, pause):
    table = np.asarray(table, np.int64)
    _engine_accepts(table, int(table[-1, 0]))
    words = _words([(0, pause[0]), (pause[1], int(table[-1, 0]))])
    rows, whole = plans.retime_rows(int(table[-1, 0]), table, words, min_pause=0)
    assert len(rows) == 2 and pause[0] <= rows[1][0] <= pause[1] and abs(rows[1][0] - sum(pause) // 2) <= 8
    _engine_accepts(whole, int(table[-1, 0]))
    for s0, sn, d0, tab in rows:
        _engine_accepts(tab, sn)
        assert sn <= 720000 and tab[-1, 1] <= 720000
    assert (plans.retime_times(table[:, 0], whole) == table[:, 1]).all()
    got = np.concatenate([s0 + plans.retime_src(np.arange(int(tab[-1, 1])), tab) for s0, _sn, _d0, tab in rows])
    assert (got == plans.retime_src(np.arange(int(whole[-1, 1])), whole)).all()


@pytest.mark.parametrize("anchors", [[[0, 0], [2000003, 250001]], [[0, 0], [250001, 2000003]], [[0, 0], [1000001, 777777]]])
def test_rows_cut_at_the_limit_pass_the_engines_checks_too(anchors):
    """No pause and no anchor: the cuts fall where max_row says, several inside ONE pair, here at rates 8 and 1/8."""
    a = np.asarray(anchors, np.int64)
    rows, whole = plans.retime_rows(int(a[-1, 0]), a, None, max_row=100000)
    assert len(rows) >= 10 and sum(r[1] for r in rows) == a[-1, 0] and sum(int(r[3][-1, 1]) for r in rows) == a[-1, 1]
    _engine_accepts(whole, int(a[-1, 0]))
    for _s0, sn, _d0, tab in rows:
        _engine_accepts(tab, sn)
        assert sn <= 100000 and tab[-1, 1] <= 100000


def test_the_engine_takes_the_rows_of_a_cut_pause_at_rate_8():
    table = np.asarray([[0, 0], [30, 30], [46, 32], [64, 50]], np.int64)
    rows, _whole = plans.retime_rows(64, table, _words([(0, 30), (46, 64)]), max_row=40, min_pause=0)
    assert len(rows) == 2
    import torch
    for s0, sn, _d0, tab in rows:
        lines, lib = _engine_call(lambda e, o: e.retime(torch.zeros(1, 1, sn), [sn], [tab], hop=16, delta=4))
        assert lib.error is None, (tab.tolist(), lib.error)
