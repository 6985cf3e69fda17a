"""CPU: the host side of the word timings — the float32 DP restatement against brute force, token groups, the mapping of
token spans onto sample timelines, the writers, the server's parameter parsing, ABI 11.  No GPU."""
import json
import re

import numpy as np
import pytest

from smalltts_amd import _lib
from smalltts_amd.api import (HOP_SIZE, Alignment, as_alignment, format_srt, plan_long, plan_packed, token_groups, word_times)
from smalltts_amd.phonemes import NV_REPEAT, p2idx
from tests.helpers import align_ref as R

# seeds for which, at every shape N, P <= 5, the brute force finds ONE cheapest path with a clear margin (checked below: a tie would
# make "equals the brute force" depend on the tie rule, which has its own test)
SEEDS = (0, 1, 2)


def _mass(seed, N, P):
    return np.random.default_rng(1000 * seed + 10 * N + P).random((N, P), dtype=np.float32)


@pytest.mark.parametrize("seed", SEEDS)
def test_float32_dp_equals_brute_force_on_every_small_grid(seed):
    for N in range(1, 6):
        for P in range(1, 6):
            mass = _mass(seed, N, P)
            cost = (np.float32(1.0) - mass).astype(np.float32)
            paths = sorted(R.brute_force_paths(cost), key=lambda cp: cp[0])
            if len(paths) > 1:   # the premise: a unique optimum, far outside fp32 summation noise (N + P <= 10 terms <= 1)
                assert paths[1][0] - paths[0][0] > 1e-5, f"seed {seed} N {N} P {P}: two paths tie, choose another seed"
            spans, score, path = R.dp_align(mass, N, 0, P)
            assert path == paths[0][1], (seed, N, P)
            assert abs(float(score) - paths[0][0]) <= (N + P) * 2.0 ** -24 * paths[0][0]
            assert np.array_equal(spans, R.spans_of_path(paths[0][1], P))
            assert path[0] == (0, 0) and path[-1] == (N - 1, P - 1)


def test_the_number_of_monotone_paths_is_the_delannoy_number():
    assert [len(R.brute_force_paths(np.zeros((n, n)))) for n in (1, 2, 3, 4)] == [1, 3, 13, 63]


def test_tie_rule_prefers_the_diagonal_then_the_previous_frame():
    """Constructed ties.  (a) every cell costs 0.5 on 3 frames x 2 tokens: D[1][0] = D[1][1] = 1.0 both feed the last cell (2,1), as
    its diagonal and its (n-1, p) predecessor — the diagonal wins.  (b) 3 x 3 with a very dear centre: the last cell's diagonal is
    out, (1,2) and (2,1) tie at 1.5 — (n-1, p) wins over (n, p-1)."""
    _, score, path = R.dp_align(np.full((3, 2), 0.5, np.float32), 3, 0, 2)
    assert path == [(0, 0), (1, 0), (2, 1)] and score == 1.5
    _, _, path = R.dp_align(np.full((2, 2), 0.5, np.float32), 2, 0, 2)
    assert path == [(0, 0), (1, 1)]
    m = np.full((3, 3), 0.5, np.float32)
    m[1, 1] = -10.0
    _, score, path = R.dp_align(m, 3, 0, 3)
    assert path == [(0, 0), (0, 1), (1, 2), (2, 2)] and score == 2.0


def test_dp_domain_prefix_and_empty_rows():
    m = _mass(7, 6, 5)
    spans, score, path = R.dp_align(m, 4, 2, 5)
    assert (spans[:2] == -1).all() and spans[2, 0] == 0 and spans[4, 1] == 3 and all(0 <= i < 4 and 2 <= t < 5 for i, t in path)
    for n, p0, p1 in ((0, 0, 5), (4, 3, 3), (4, 4, 2)):
        spans, score, path = R.dp_align(m, n, p0, p1)
        assert (spans == -1).all() and score == 0 and path == []
    spans, _, path = R.dp_align(m, 1, 0, 5)          # one frame speaks every token
    assert (spans == 0).all() and len(path) == 5


def test_token_groups_words_punctuation_events_and_spaces():
    sp = p2idx[" "]
    ev = p2idx["[laughter]"]
    w = lambda s: [p2idx[c] for c in s]
    ids = [sp] + w("hɛ") + [sp, sp] + w("wˈɜːld") + w(",") + [sp] + [ev] * NV_REPEAT + w("ok") + w("!") + w("?") + [0, 0]
    g = token_groups(ids)
    assert [(k, ph) for k, ph, _, _ in g] == [("word", "hɛ"), ("word", "wˈɜːld"), ("punct", ","), ("event", "[laughter]"),
                                              ("word", "ok"), ("punct", "!"), ("punct", "?")]
    assert [(t0, t1) for _, _, t0, t1 in g] == [(1, 3), (5, 11), (11, 12), (13, 13 + NV_REPEAT), (17, 19), (19, 20), (20, 21)]
    assert all(ids[t] != sp and ids[t] != 0 for _, _, t0, t1 in g for t in range(t0, t1))
    # two events in a row are two groups; a longer run of one event id is cut every NV_REPEAT copies
    g = token_groups([ev] * (NV_REPEAT + 1) + [p2idx["[sigh]"]] * NV_REPEAT)
    assert [(k, t0, t1) for k, _, t0, t1 in g] == [("event", 0, NV_REPEAT), ("event", NV_REPEAT, NV_REPEAT + 1),
                                                   ("event", NV_REPEAT + 1, 2 * NV_REPEAT + 1)]
    assert token_groups([]) == [] and token_groups([sp, sp, 0]) == []


def test_word_times_hand_arithmetic_plain_trimmed_and_offset():
    groups = [("word", "a", 0, 2), ("punct", ",", 2, 3), ("word", "b", 4, 6)]          # token 3 is a space
    spans = np.array([[0, 1], [1, 1], [2, 2], [2, 3], [3, 5], [6, 9]], np.int32)
    # plain: start = 3200 * first(t0), end = 3200 * (last(t1 - 1) + 1), clipped to 3200 * n
    assert word_times(groups, spans, 10) == [(0, "word", 0, 6400), (1, "punct", 6400, 9600), (2, "word", 9600, 32000)]
    assert word_times(groups, spans, 8)[2] == (2, "word", 9600, 25600)                   # the row ends at frame 8
    # a speech window (start 5000, n 20000): intersect, then count from its start
    assert word_times(groups, spans, 10, window=(5000, 20000)) == [(0, "word", 0, 1400), (1, "punct", 1400, 4600), (2, "word", 4600, 20000)]
    # entirely in front of the window -> collapses to its start; offset and index0 shift the lot
    assert word_times(groups, spans, 10, window=(9600, 3200), offset=100000, index0=7) == [
        (7, "word", 100000, 100000), (8, "punct", 100000, 100000), (9, "word", 100000, 103200)]
    # a prepended transcription of 3 tokens: the groups index the text's own tokens
    sp3 = np.concatenate([np.full((3, 2), -1, np.int32), spans])
    assert word_times(groups, sp3, 10, token0=3) == word_times(groups, spans, 10)
    # an empty row: every span is (-1, -1)
    assert word_times(groups, np.full((6, 2), -1, np.int32), 0, offset=50) == [(0, "word", 50, 50), (1, "punct", 50, 50), (2, "word", 50, 50)]


def test_word_times_on_the_long_form_timelines_with_gaps():
    """pieces of 3 and 2 frames, 120 ms apart (plan_long), then the same with speech windows (plan_packed)."""
    g1, g2 = [("word", "a", 0, 1), ("word", "b", 1, 2)], [("word", "c", 0, 1)]
    s1, s2 = np.array([[0, 0], [1, 2]], np.int32), np.array([[0, 1]], np.int32)
    _, offs, S = plan_long([3, 2], 8, 120.0)
    assert offs == [0, 3 * HOP_SIZE + 2880] and S == 5 * HOP_SIZE + 2880
    words = word_times(g1, s1, 3, offset=offs[0])
    words += word_times(g2, s2, 2, offset=offs[1], index0=len(words))
    assert words == [(0, "word", 0, 3200), (1, "word", 3200, 9600), (2, "word", 12480, 18880)]
    wins = [(1000, 7000), (200, 6000)]
    poffs, S = plan_packed([n for _, n in wins], 120.0)
    assert poffs == [0, 7000 + 2880] and S == 7000 + 2880 + 6000
    words = word_times(g1, s1, 3, window=wins[0], offset=poffs[0])
    words += word_times(g2, s2, 2, window=wins[1], offset=poffs[1], index0=len(words))
    assert words == [(0, "word", 0, 2200), (1, "word", 2200, 7000), (2, "word", 9880, 9880 + 6000)]
    starts = [w[2] for w in words]
    assert starts == sorted(starts)


def test_alignment_options_object():
    a = Alignment()
    assert (a.layers, a.heads, a.steps) == (None, None, None) and as_alignment(True) == a and as_alignment(None) is None
    assert as_alignment(False) is None and as_alignment(a) is a
    b = Alignment(layers=[5, 3, 3], heads=(0,), steps=[-1])
    assert b.layers == (3, 5) and b.heads == (0,) and b.steps == (-1,) and b != a and hash(b) == hash(Alignment([3, 5], [0], [-1]))
    with pytest.raises(AttributeError):
        a.layers = (1,)
    for bad in (dict(layers=[12]), dict(heads=[-1]), dict(layers=[]), dict(steps=[])):
        with pytest.raises(ValueError):
            Alignment(**bad)
    with pytest.raises(TypeError):
        as_alignment("yes")
    assert "unvalidated" in Alignment.__doc__.lower()


def test_tap_selection_masks_and_step_flags():
    from smalltts_amd.engine import tap_selection
    flags, layers, heads = tap_selection(True, 4)
    assert list(flags) == [0, 0, 0, 1] and layers == 0xFFF and heads == 0xFF
    flags, layers, heads = tap_selection(Alignment(layers=[0, 11], heads=[2], steps=[0, -1]), 4)
    assert list(flags) == [1, 0, 0, 1] and layers == 0x801 and heads == 0x4
    with pytest.raises(ValueError):
        tap_selection(Alignment(steps=[4]), 4)
    with pytest.raises(TypeError):
        tap_selection(object(), 4)


def test_srt_and_json_writers():
    from smalltts_amd.scripts.longform import group_texts, piece_cues, word_cues, words_json
    srt = format_srt([(0, 24000, "one"), (24000, 24000 + 36, ""), (90_000_000, 90_012_000, "two\n")])
    assert srt == "1\n00:00:00,000 --> 00:00:01,000\none\n\n2\n01:02:30,000 --> 01:02:30,500\ntwo\n"
    assert format_srt([(12, 0, "x")]).splitlines()[1] == "00:00:00,001 --> 00:00:00,001"     # 12 samples = 0.5 ms rounds up; end >= start
    assert format_srt([]) == ""
    toks = [[p2idx["a"], p2idx[" "], p2idx["b"]], [p2idx["!"]]]
    texts = group_texts(toks)
    assert texts == [(0, "word", "a"), (0, "word", "b"), (1, "punct", "!")]
    words = [(0, "word", 0, 3200), (1, "word", 3200, 9600), (2, "punct", 12480, 18880)]
    doc = json.loads(words_json(words, texts))
    assert [d["phonemes"] for d in doc] == ["a", "b", "!"] and doc[2] == {"index": 2, "piece": 1, "kind": "punct", "phonemes": "!",
                                                                          "start": 12480, "end": 18880, "start_s": 0.52, "end_s": 0.7867}
    with pytest.raises(ValueError):
        words_json(words[:2], texts)
    assert piece_cues([(0, 9600, 0, 1.0), (12480, 0, 0, 1.0)], ["a b", "!"]) == [(0, 9600, "a b")]
    assert word_cues(words, texts)[1] == (3200, 9600, "b")


def test_server_align_parameter_and_header_cap():
    from smalltts_amd import server as S
    assert S.parse_align_query({}) is False and S.parse_align_query({"align": ["0"]}) is False
    assert S.parse_align_query({"align": ["1"]}, 10.0, [1] * 198) is True and S.parse_align_query({"align": ["true"]}) is True
    for q, dur, toks in (({"align": ["yes"]}, 1.0, [1]), ({"align": ["1"]}, 30.1, [1]), ({"align": ["1"]}, 1.0, [1] * 199)):
        with pytest.raises(S.HttpError) as e:
            S.parse_align_query(q, dur, toks)
        assert e.value.code == 400 and "align" in e.value.msg
    assert S.parse_align_query({"align": ["0"]}, 300.0, [1] * 4000) is False            # off: no new limit
    assert S.words_header([(0, "word", 0, 3200), (1, "punct", 3200, 6400)]) == "[[0,3200],[3200,6400]]"
    many = [(i, "word", 700000 + i, 700001 + i) for i in range(400)]
    assert len(S.words_header(many[:300])) <= S.WORDS_HEADER_LIMIT == 6144
    with pytest.raises(S.HttpError) as e:
        S.words_header(many)
    assert e.value.code == 400 and "6144" in e.value.msg
    r = S.Request(None, 24000, [1], 1.0, 0)
    assert r.align is False and r.trim is None


def test_abi_11_header_and_host_agree():
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    assert _lib.ABI_VERSION == 11 and re.search(r"#define\s+SMTTS_ABI_VERSION\s+(\d+)", txt).group(1) == "11"
    for name in ("smtts_sample_align", "smtts_align_path", "smtts_test_attn_text_mass"):
        assert name in _lib.SIGNATURES and name in _lib.header_symbols(), name
        assert _lib.SIGNATURES[name][1][0] is _lib.vp
    # smtts_sample keeps its signature; smtts_sample_align is that list plus (tap_steps, tap_layers, tap_heads, text_mass)
    assert _lib.SIGNATURES["smtts_sample_align"][1][:-4] == _lib.SIGNATURES["smtts_sample"][1]
    assert len(_lib.SIGNATURES["smtts_sample"][1]) == 24
    assert _lib.SIGNATURES["smtts_test_attn_text_mass"][1] == _lib.SIGNATURES["smtts_test_attention_mfma"][1]
    assert "trained weights has not been measured" in re.sub(r"[\s*]+", " ", txt)     # the limit stays visible at the boundary
