"""CPU: pitch (include/smalltts_hip.h smtts_pitch).  The numpy restatement of tests/helpers/pitch_ref.py on synthetic
signals (the conditions tests/test_pitch_gpu.py then holds the device to), broken copies of it that must fail those conditions, the host
arithmetic of plans.py and options.py, what HipEngine.pitch hands to the C ABI (against the stand-in library), and the retime / pitch
yardstick: how far the reference's own track of a retimed signal lies from its track of the input.  Synthetic signals only: nothing here
says anything about speech."""
import json
import re
import subprocess
import sys

import numpy as np
import pytest

from smalltts_amd import _lib, options, plans
from tests.helpers import pitch_ref as R
from tests.helpers import retime_ref as RT

LONG_390 = dict(f0=390.0, n=72000, on=3600, off=68400)          # 2.7 s of tone: long enough for an octave error to pay its jump


@pytest.fixture(scope="module")
def tones():
    """Each tone's reference track, computed once."""
    out = {}
    for f0 in R.TONES:
        x = R.tone_case(f0)
        out[f0] = (x,) + R.track(x, x.size, R.DEFAULT)
    return out


@pytest.fixture(scope="module")
def long_tone():
    c = LONG_390
    return R.tone(c["f0"], c["n"], c["on"], c["off"], None, seed=1)


def _check_long(lag):
    c = LONG_390
    return R.check_tone(lag, R.DEFAULT, c["n"], c["on"], c["off"], None, R.SR / c["f0"])


# ---- 1. the reference on synthetic signals -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("f0", R.TONES)
def test_a_tone_is_voiced_at_its_period_and_silence_is_unvoiced(tones, f0):
    x, lag, peak, S = tones[f0]
    n_tone, n_quiet = R.check_tone(lag, R.DEFAULT, x.size, R.TONE_ON, R.TONE_OFF, R.TONE_HOLE, R.SR / f0)
    assert n_tone >= 80 and n_quiet >= 25
    voiced = lag > 0
    assert (peak[~voiced] == 0).all() and (peak[voiced, 1] == S[voiced, lag[voiced] - R.DEFAULT.lmin]).all()
    f, strength = plans.pitch_f0(lag, peak)
    inner = R.inside(R.DEFAULT, x.size, [(R.TONE_ON, R.TONE_HOLE[0]), (R.TONE_HOLE[1], R.TONE_OFF)])
    # one step of the lag grid is f0^2 / sr Hz; the parabola does better, but nothing finer is claimed
    assert (np.abs(f[inner] - f0) <= f0 * f0 / R.SR + 1e-9).all() and (strength[inner] > 0.9).all() and (f[~voiced] == 0).all()


def test_a_long_tone_keeps_its_octave(long_tone):
    _check_long(R.track(long_tone, long_tone.size, R.DEFAULT)[0])


@pytest.mark.parametrize("period", R.TINY_PERIODS)
def test_the_same_at_the_tiny_shape(period):
    x = R.tiny_case(period)
    lag, _peak, _S = R.track(x, x.size, R.TINY)
    R.check_tone(lag, R.TINY, x.size, R.TINY_ON, R.TINY_OFF, None, period)


@pytest.mark.parametrize("P,n", [(R.DEFAULT, 24000), (R.TINY, 1600)])
def test_white_noise_has_no_voiced_frame(P, n):
    lag, _peak, _S = R.track(R.white(5, n), n, P)
    assert lag.shape == (P.frames(n),) and (lag == 0).all()


def test_silence_scores_zero_and_the_floor_scores_next_to_nothing():
    P = R.DEFAULT
    S, E = R.scores(np.zeros((4800,), np.float32), 4800, P)
    assert S.shape == (20, P.L) and (S == 0).all() and (E == 0).all()
    # a 1e-4 floor: e0, e ~ win * 1e-8, so |S| <= sqrt(e0 e / (e0 e + bias)) ~ 1e-8 / 1e-6 = 0.01; twice that allows for the energies' spread
    S, _E = R.scores(R.white(3, 4800, 1e-4), 4800, P)
    assert np.abs(S).max() < 0.02


def test_samples_behind_len_read_as_zero_and_the_bound_is_small():
    x = R.tone_case(220.0)
    n = 7001                                                     # no multiple of hop
    S, E = R.scores(x, n, R.DEFAULT)
    y = x.copy()
    y[n:] = np.nan
    S2, _E = R.scores(y, n, R.DEFAULT)
    assert S.shape == (30, R.DEFAULT.L) and np.array_equal(S, S2) and (S[-1, :] == S[-1, :]).all()
    assert E.max() < 2 * (2 * 482 + 4) * R.U * 1.0001            # |S| <= 1 and sum |x y| <= den: at most 2 (2 g + 4 u)


# ---- 2. the path on crafted scores ---------------------------------------------------------------------------------------------------
def _flat(P, F, value):
    tab = np.stack([np.zeros((P.L,), np.float32), np.ones((P.L,), np.float32)])   # every lag alike: lg 0, tilt 1
    return np.full((F, P.L), value, np.float32), tab


def test_ties_go_to_the_smallest_state(ties="smallest"):
    S, tab = _flat(R.TINY, 6, 0.9)
    lag, peak = R.path(S, R.TINY, tab=tab, ties=ties)
    assert (lag == R.TINY.lmin).all() and (peak == np.float32(0.9)).all()


def test_an_isolated_weak_frame_does_not_switch_voicing(w_switch=None):
    P = R.TINY
    S = np.zeros((9, P.L), np.float32)
    S[4, 5] = 0.6                                                # 0.4 < c_unv by 0.15, two switches cost 0.6
    lag, peak = R.path(S, P, w_switch=w_switch)
    assert (lag == 0).all() and (peak == 0).all()
    S[2:7, 5] = 0.9                                              # five strong frames gain 5 * (0.55 - 0.1...) > 0.6
    lag, _peak = R.path(S, P, w_switch=w_switch)
    assert (lag[2:7] == P.lmin + 5).all() and (lag[:2] == 0).all() and (lag[7:] == 0).all()


def test_a_nan_score_is_never_chosen_and_the_table_is_clamped():
    P = R.TINY
    S = np.full((5, P.L), 0.95, np.float32)
    S[:, :10] = np.nan
    lag, peak = R.path(S, P)
    assert (lag == P.lmin + 10).all() and not np.isnan(peak[:, 1:]).any() and np.isnan(peak[:, 0]).all()
    tab = P.tab.copy()
    tab[0, 3], tab[1, 4], tab[0, 7], tab[1, 8] = np.nan, np.nan, np.inf, -5.0
    lg, tilt = R.tables(tab, P.L)
    assert lg[3] == 0 and tilt[4] == 0 and lg[7] == 16 and tilt[8] == 0
    assert R.path(np.full((5, P.L), np.nan, np.float32), P)[0].tolist() == [0] * 5     # state 0 is always there
    assert R.path(np.zeros((0, P.L), np.float32), P)[0].shape == (0,)
    one = R.path(np.full((1, P.L), 0.9, np.float32), P)[0]
    assert one.tolist() == [P.lmin]                              # one frame: the end rule alone


# ---- 3. broken copies of the reference fail the checks above -------------------------------------------------------------------------
def test_without_the_tilt_the_long_tone_drops_an_octave(long_tone):
    lag, _peak, _S = R.track(long_tone, long_tone.size, R.Shape(tilt=0.0))
    with pytest.raises(AssertionError, match="lag off the period"):
        _check_long(lag)
    assert np.bincount(lag).argmax() == 123                      # two periods of 61.5 samples


def test_ties_to_the_largest_state_fail():
    with pytest.raises(AssertionError):
        test_ties_go_to_the_smallest_state(ties="largest")


def test_without_the_switch_cost_the_weak_frame_switches():
    with pytest.raises(AssertionError):
        test_an_isolated_weak_frame_does_not_switch_voicing(w_switch=0.0)


def test_without_the_bias_silence_does_not_score_zero():
    S, _E = R.scores(np.zeros((4800,), np.float32), 4800, R.DEFAULT, bias=0.0)
    assert np.isnan(S).all()
    S, _E = R.scores(R.white(3, 4800, 1e-4), 4800, R.DEFAULT, bias=0.0)
    assert np.nanmax(np.abs(S)) > 0.02                           # ... and the floor scores like any noise (NaN behind the end)


# ---- 4. plans.py and options.py ------------------------------------------------------------------------------------------------------
def test_the_tables():
    for P in R.SHAPES.values():
        t = plans.pitch_tables(P.lmin, P.lmax, 0.1)
        assert t.dtype == np.float32 and t.shape == (2, P.L) and np.array_equal(t, P.tab)
    t = plans.pitch_tables(60, 400)
    assert t[0, 4] == 6.0 and t[1, 0] == 1.0 and t[1, -1] == np.float32(0.9)
    for bad in ((0, 5, 0.1), (5, 5, 0.1), (5, 9, 1.0), (5, 9, -0.1)):
        with pytest.raises(ValueError, match="pitch_tables"):
            plans.pitch_tables(*bad)


def test_f0_from_exact_parabolas():
    # S(l) = 1 - k (l - v)^2 sampled at 99, 100, 101 has its vertex at v
    lags, verts, ks = [100, 100, 100, 100], [100.0, 100.25, 99.6, 100.5], [0.01, 0.02, 0.005, 0.01]
    peak = np.asarray([[1 - k * (l - 1 - v) ** 2, 1 - k * (l - v) ** 2, 1 - k * (l + 1 - v) ** 2] for l, v, k in zip(lags, verts, ks)],
                      np.float64)
    f0, strength = plans.pitch_f0(np.asarray(lags, np.int32), peak)
    assert f0.dtype == np.float64 and strength.dtype == np.float32
    assert np.abs(f0 - 24000.0 / np.asarray(verts)).max() < 24000.0 / 100.0 ** 2 * 2e-5        # fp32 triples: 1e-7 / k of a lag
    # clamped, flat, not a maximum, unvoiced
    lag = np.asarray([100, 100, 100, 100, 0], np.int32)
    peak = np.asarray([[0.2, 0.5, 0.9], [0.5, 0.5, 0.5], [0.9, 0.5, 0.9], [0.9, 0.95, 0.2], [0, 0, 0]], np.float32)
    f0, strength = plans.pitch_f0(lag, peak, sr=16000)
    assert f0.tolist()[:3] == [160.0, 160.0, 160.0] and f0[4] == 0 and strength.tolist() == peak[:, 1].tolist()
    a, b, c = (np.float64(np.float32(v)) for v in (0.9, 0.95, 0.2))
    d = 0.5 * (a - c) / (a - 2 * b + c)
    assert -0.5 <= d < 0 and f0[3] == 16000.0 / (100 + d)
    assert plans.pitch_f0(np.asarray([80], np.int32), np.asarray([[0.1, 0.5, 0.9]]))[0][0] == 24000.0 / 80.0   # no maximum: d = 0
    assert plans.pitch_f0(np.asarray([80], np.int32), np.asarray([[0.5, 0.9, 0.9]]))[0][0] == 24000.0 / 80.5       # d = 0.5, the clamp's edge
    two = plans.pitch_f0(np.zeros((2, 3), np.int32), np.zeros((2, 3, 3), np.float32))
    assert two[0].shape == (2, 3) and two[1].shape == (2, 3)
    with pytest.raises(ValueError, match="pitch_f0"):
        plans.pitch_f0(np.zeros((3,), np.int32), np.zeros((3, 2), np.float32))


def test_word_stats():
    f0 = np.asarray([0, 100, 110, 0, 120, 0, 0, 200, 0, 0], np.float64)            # hop 10: frame f starts at 10 f
    words = [(0, "word", "a", 10, 50, -0.1), (1, "punct", ",", 50, 50, -0.1), (2, "word", "b", 50, 70, -0.2), (3, "word", "c", 65, 100, 0.0),
             (4, "word", "d", 95, 400, 0.0)]
    st = plans.pitch_word_stats(words, f0, 10)
    assert st[0] == dict(f0_median=110.0, f0_min=100.0, f0_max=120.0, voiced=0.75)  # frames 1 .. 4
    assert st[1] == dict(f0_median=None, f0_min=None, f0_max=None, voiced=0.0)      # an empty span
    assert st[2] == dict(f0_median=None, f0_min=None, f0_max=None, voiced=0.0)      # frames 5, 6: none voiced
    assert st[3] == dict(f0_median=200.0, f0_min=200.0, f0_max=200.0, voiced=1 / 3) # frames 7 .. 9 (65 -> the frame that starts at 70)
    assert st[4]["voiced"] == 0.0                                                     # behind the track
    assert plans.pitch_word_stats([(0, "word", 10, 50)], f0, 10)[0]["f0_median"] == 110.0   # synthesize_long's four columns
    with pytest.raises(ValueError, match="pitch_word_stats"):
        plans.pitch_word_stats(words, f0, 0)


@pytest.mark.parametrize("n,hop", [(720000, 240), (720001, 240), (31 * 24000, 240), (5000000, 240), (3 * 720000 + 17, 16), (100, 240),
                                   (2 * 720000 - 24000, 240), (2 * 720000 - 24000 + 1, 240)])
def test_rows_cover_every_frame_once(n, hop):
    rows = plans.pitch_rows(n, hop)
    F = -(-n // hop)
    assert rows[0][0] == 0 and rows[0][2] == 0 and rows[-1][0] + rows[-1][1] == n
    assert sum(r[3] for r in rows) == F and all(r[3] >= 1 for r in rows)
    for k, (s0, sn, f0, fn) in enumerate(rows):
        assert s0 % hop == 0 and 1 <= sn <= plans.PITCH_MAX_ROW                      # cuts on multiples of hop, rows of 30 s at most
        assert f0 == (rows[k - 1][2] + rows[k - 1][3] if k else 0)                   # in order, without a gap
        lo, hi = s0 // hop, s0 // hop + -(-sn // hop)                                # the row's own frames
        assert lo <= f0 and f0 + fn <= hi
        if k:                                                                        # the shared second, split in the middle
            p0, pn = rows[k - 1][0], rows[k - 1][1]
            shared = (p0 + pn - s0) // hop
            assert shared == plans.PITCH_CONTEXT // hop // 2 * 2 and f0 - lo == shared // 2
            # ownership: a kept frame lies at least as far from its own row's cuts as from the neighbour's
            assert f0 - lo >= 0 and (p0 + pn) // hop - f0 == shared - shared // 2
    if n <= plans.PITCH_MAX_ROW:
        assert rows == [(0, n, 0, F)]


def test_rows_at_other_limits_and_refusals():
    rows = plans.pitch_rows(1000, 10, max_row=400, context=100)
    assert rows == [(0, 400, 0, 35), (300, 400, 35, 30), (600, 400, 65, 35)]
    for bad in (dict(n=0, hop=10), dict(n=10, hop=0), dict(n=100, hop=10, max_row=30), dict(n=100, hop=10, max_row=100, context=80)):
        with pytest.raises(ValueError, match="pitch_rows"):
            plans.pitch_rows(**bad)


def test_the_pitch_option():
    p = options.Pitch()
    assert (p.fmin, p.fmax, p.hop, p.win, p.floor_pow, p.tilt, p.c_unv, p.w_jump, p.w_switch) == (60.0, 400.0, 240, 480, 1e-6, 0.1, 0.55,
                                                                                                  0.35, 0.3)
    assert (p.lmin, p.lmax) == (60, 400) and p.bias == (480 * 1e-6) ** 2 and np.float32(p.bias) == R.DEFAULT.bias
    assert p == options.Pitch(fmin=60) and p != options.Pitch(fmin=61) and hash(p) == hash(options.Pitch())
    assert options.Pitch(fmin=70.0, fmax=390.0).lmin == 61 and options.Pitch(fmin=70.0, fmax=390.0).lmax == 343   # floor, ceil
    assert options.Pitch(fmin=600, fmax=3000, hop=16, win=64).lmax == 40
    with pytest.raises(AttributeError):
        p.hop = 3
    for bad in (dict(hop=12), dict(hop=1028), dict(hop=242), dict(win=28), dict(win=2052), dict(win=482), dict(fmin=0), dict(fmin=400),
                dict(fmax=12001), dict(fmin=11), dict(fmin=20, fmax=12000), dict(floor_pow=0), dict(floor_pow=float("nan")),
                dict(tilt=1.0), dict(tilt=-0.1), dict(c_unv=-1), dict(w_jump=-0.1), dict(w_switch=float("inf"))):
        with pytest.raises(ValueError, match="Pitch: "):
            options.Pitch(**bad)
    for bad in (dict(hop=240.0), dict(win=True), dict(fmin="60"), dict(c_unv=None)):
        with pytest.raises(TypeError, match="Pitch: "):
            options.Pitch(**bad)
    assert options.as_pitch(None) == p and options.as_pitch(p) is p
    with pytest.raises(TypeError, match="pitch must be"):
        options.as_pitch(1.5)
    assert "synthetic signals only" in options.Pitch.__doc__


def test_options_and_plans_still_import_without_torch():
    code = ("import sys\nfrom smalltts_amd.options import Pitch\nfrom smalltts_amd import plans\n"
            "assert Pitch().lmax == 400 and plans.pitch_tables(8, 40).shape == (2, 33) and len(plans.pitch_rows(10 ** 6, 240)) == 2\n"
            "assert 'torch' not in sys.modules and 'smalltts_amd.engine' not in sys.modules\nprint('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]


# ---- 5. the C ABI's two lists, and what the engine hands to it --------------------------------------------------------------------------
def test_the_entries_are_in_the_signature_table_and_in_the_header():
    assert _lib.ABI_VERSION == 11
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    assert "synthetic signals only" in txt
    for name, ret, res_t, count in (("smtts_pitch", "int", _lib.i32, 20), ("smtts_pitch_workspace_bytes", "size_t", _lib.sz, 6)):
        assert name in _lib.SIGNATURES and name in _lib.header_symbols()
        res, args = _lib.SIGNATURES[name]
        decl = txt[txt.index(f"{ret} {name}("):]
        decl = decl[:decl.index(";")]
        params = re.sub(r"/\*.*?\*/", "", decl[decl.index("(") + 1: decl.rindex(")")], flags=re.S).split(",")
        assert res is res_t and len(args) == len(params) == count
        kinds = [_lib.vp if "*" in p or "smtts_handle" in p else _lib.i64 if "int64_t" in p else _lib.sz if "size_t" in p
                 else _lib.f32 if "float" in p else _lib.i32 for p in params]
        assert kinds == args, name


def _engine_call(fn, **opts):
    import smalltts_amd.engine  # noqa: F401  (the stand-in patches the modules that are loaded when it is entered)
    from tests.helpers.engine_cases import operands
    from tests.helpers.engine_standin import record
    return record("pitch", fn, operands(), **opts)


SMALL = dict(fmin=600, fmax=3000, hop=16, win=64)                # the tiny shape: lags 8 .. 40


def test_engine_pitch_asks_for_the_workspace_and_makes_one_call():
    lines, lib = _engine_call(lambda e, o: e.pitch(o.audio, [40, 24], options.Pitch(**SMALL), return_nccf=True))
    assert lib.error is None and [l.split(" ")[0] for l in lines if l.startswith("smtts_")] == ["smtts_pitch_workspace_bytes", "smtts_pitch"]
    assert lines[1].split(" ")[1:] == ["h", "2", "64", "16", "8", "40"]
    call = lines[2].replace("tmp:float32(2, 33)", "tab").split(" ")         # (the cached table is neither an operand nor a result)
    # h stream audio B row_stride len tab hop win lmin lmax bias c_unv w_jump w_switch lag peak nccf ws ws_bytes
    assert call[1:8] == ["h", "stream", "audio+0", "2", "64", "table0+0", "tab"] and call[8:12] == ["16", "64", "8", "40"]
    assert [float(v) for v in call[12:16]] == [(64 * 1e-6) ** 2, 0.55, 0.35, 0.3]          # (ctypes rounds them to fp32)
    assert call[16:] == ["ret[0]+0", "ret[1]+0", "ret[2]+0", "ws+0", "256"]
    assert lines[3] == "table0 int64(2,) [40, 24]"
    assert lines[-1] == "-> (int32(2, 4), float32(2, 4, 3), float32(2, 4, 33))"
    lines, lib = _engine_call(lambda e, o: (e.pitch(o.audio, [40, 24], options.Pitch(**SMALL)), e.pitch(o.audio, [0, 64], options.Pitch(**SMALL)),
                                            e.pitch(o.audio, [1, 2])))
    calls = [args for name, args in lib.calls if name == "smtts_pitch"]
    assert lib.error is None and len(calls) == 3
    assert calls[0][6].tensor is calls[1][6].tensor and calls[0][6].tensor is not calls[2][6].tensor    # the table: cached per shape
    assert tuple(calls[0][6].tensor.shape) == (2, 33) and np.array_equal(calls[0][6].tensor.numpy(), R.TINY.tab)
    assert calls[0][17] == "null" and calls[2][7:11] == ["240", "480", "60", "400"]                    # no nccf; None: the defaults


def test_engine_pitch_refuses():
    for fn, match in ((lambda e, o: e.pitch(o.audio, [40, 65]), "lengths"),
                      (lambda e, o: e.pitch(o.audio, [40]), "lengths"),
                      (lambda e, o: e.pitch(o.audio, [-1, 3]), "lengths"),
                      (lambda e, o: e.pitch(o.audio.new_zeros(1025, 1, 16), [16] * 1025), "at most 1024 rows"),
                      (lambda e, o: e.pitch(o.audio2, [40, 24]), r"\(B,1,S\)"),
                      (lambda e, o: e.pitch(o.audio.double(), [40, 24]), r"\(B,1,S\)"),
                      (lambda e, o: e.pitch(o.audio[:, :, ::2], [20, 24]), r"\(B,1,S\)")):
        lines, lib = _engine_call(fn)
        assert isinstance(lib.error, ValueError) and str(lib.error).startswith("pitch: ") and not lib.calls, lib.error
        assert re.search(match, str(lib.error)), lib.error
    lines, lib = _engine_call(lambda e, o: e.pitch(o.audio, [40, 24]), zero=["smtts_pitch_workspace_bytes"])
    assert isinstance(lib.error, RuntimeError) and str(lib.error).startswith("pitch: ")
    assert [name for name, _a in lib.calls if name not in ("smtts_last_error",)] == ["smtts_pitch_workspace_bytes"]
    lines, lib = _engine_call(lambda e, o: e.pitch(o.audio, [40, 24]), fail=["smtts_pitch"])
    assert isinstance(lib.error, RuntimeError) and str(lib.error).startswith("pitch: ")


def test_engine_pitch_takes_a_pitch_or_none_only():
    import smalltts_amd.engine  # noqa: F401
    from tests.helpers.engine_cases import operands
    from tests.helpers.engine_standin import StandinLib, make_engine, standin
    lib = StandinLib()
    with standin(lib, []):
        eng = make_engine(lib)
        with pytest.raises(TypeError, match="pitch must be"):
            eng.pitch(operands().audio, [40, 24], pitch=1.5)
    assert not lib.calls


# ---- 6. the layers above, as far as they are host arithmetic ---------------------------------------------------------------------------
def test_the_api_names_and_the_command_lines(tmp_path):
    from smalltts_amd import api
    from smalltts_amd.scripts import align, pitch as cli
    for name in ("Pitch", "as_pitch", "PitchTrack", "pitch_track", "pitch_track_wav", "pitch_f0", "pitch_rows", "pitch_word_stats"):
        assert hasattr(api, name)
    assert hasattr(api.SmallTTS, "pitch") and hasattr(api.SmallTTS, "pitch_wav")
    assert "synthetic signals only" in api.pitch_track.__doc__ and "synthetic signals only" in cli.__doc__
    rows = [(0, "word", "ab", 0, 800, -0.5), (1, "punct", ",", 800, 800, float("-inf"))]
    plain = align.words_json(rows)
    assert align.words_json(rows, None) == plain and "f0_median" not in plain      # without --pitch the file keeps its bytes
    assert [sorted(r) for r in json.loads(plain)] == [sorted(["index", "kind", "phonemes", "start", "end", "start_s", "end_s", "confidence"])] * 2
    stats = [dict(f0_median=110.123, f0_min=100.0, f0_max=120.0, voiced=0.75), dict(f0_median=None, f0_min=None, f0_max=None, voiced=0.0)]
    got = json.loads(align.words_json(rows, stats))
    assert [{k: r[k] for k in json.loads(plain)[i]} for i, r in enumerate(got)] == json.loads(plain)
    assert got[0]["f0_median"] == 110.12 and got[0]["voiced"] == 0.75 and got[1]["f0_min"] is None and got[1]["voiced"] == 0.0
    spans = np.asarray([[0, 3], [4, 9]])
    assert align.long_json(rows, spans, None) == align.long_json(rows, spans)
    assert json.loads(align.long_json(rows, spans, stats))["words"] == got
    track = api.PitchTrack(np.asarray([0.0, 110.1234]), np.asarray([0.0, 0.98768], np.float32), 240, 24000)
    doc = json.loads(cli.pitch_json(track, list(zip(rows, stats))))
    assert doc["hop"] == 240 and doc["sr"] == 24000 and doc["f0"] == [0.0, 110.123] and doc["strength"] == [0.0, 0.9877]
    assert doc["words"] == got and "words" not in json.loads(cli.pitch_json(track))
    for bad in (["--wav", "a.wav"], ["--out", "o.json"], ["--wav", "a.wav", "--out", str(tmp_path / "o.json"), "--fmin", "500"],
                ["--wav", "a.wav", "--out", str(tmp_path / "o.json"), "--fmin", "5"]):
        with pytest.raises(SystemExit):
            cli.main(bad)
    for bad in (["--wav", "a.wav", "--text", "x", "--srt", "o.srt", "--pitch"], ["--take", "t.npz", "--out-take", "o.npz", "--pitch"]):
        with pytest.raises(SystemExit):
            align.main(bad)


# ---- 7. the retime / pitch yardstick ----------------------------------------------------------------------------------------------------
def test_the_references_track_of_a_retimed_signal_stays_within_d_ref():
    """WSOLA keeps the pitch: the reference's track of retime_ref's output, frame f, against its track of the input at frame round(f *
    speed).  The worst deviation over the inner frames is D_REF = 2 lags at both speeds, with every compared frame voiced;
    tests/test_pitch_gpu.py allows the device D_REF + 1."""
    P = R.DEFAULT
    x = RT.voiced_signal(3, 48000)
    lag_in = R.track(x, x.size, P)[0]
    assert (lag_in[2:-4] > 0).all()
    worst = []
    for speed in R.YARD_SPEEDS:
        n_out = int(round(x.size / speed))
        out = RT.retime_row(x, x.size, np.asarray([[0, 0], [x.size, n_out]]), 2, RT.window(240), 240, 120, n_out)["out"]
        d, unvoiced, pairs = R.yardstick(lag_in, R.track(out, n_out, P)[0], P, x.size, n_out, speed)
        print(f"speed {speed}: {pairs} frames compared, worst deviation {d} lags, {unvoiced} unvoiced")
        assert unvoiced == 0 and pairs >= 150
        worst.append(d)
    assert max(worst) == R.D_REF and worst == [2, 2]
