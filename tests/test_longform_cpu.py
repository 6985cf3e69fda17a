"""CPU: the host side of long-form synthesis: the text splitter, the numpy statement of the stitch the GPU kernel is held to, the
planner of synthesize_long, and the three new C entries in the header.  No GPU, no espeak (count_tokens=len)."""
import re

import numpy as np
import pytest

from smalltts_amd import _lib
from smalltts_amd.api import CHARS_PER_SECOND, HOP_SIZE, fade_table, piece_seed, plan_long, split_text
from tests.helpers.longform_ref import STITCH_CASES, stitch_case, stitch_naive, stitch_numpy

TAG = re.compile(r"\[(\w+)\]")

FIXED = [
    "Hello there. This is a test! Is it working? Yes… it is.",
    "One very long sentence, with a clause here, and another clause there; then a third: all of it without a full stop",
    "  Leading and   trailing\twhitespace\n\nand a [laughter] tag. Then [cough] more words, [sigh]. ",
    "short",
    "A. B. C. D. E. F. G. H.",
]


def _check(text, pieces, max_tokens, max_seconds):
    assert " ".join(pieces) == " ".join(text.split())
    for p in pieces:
        assert p and p == p.strip()
        assert len(p) <= max_tokens and len(p) / CHARS_PER_SECOND <= max_seconds, (p, len(p))
    # no piece begins or ends inside a tag: the tags of the pieces are the tags of the text, in order, and none is left open
    assert [m for p in pieces for m in TAG.findall(p)] == TAG.findall(text)
    for p in pieces:
        assert TAG.sub("", p).count("[") == 0 and TAG.sub("", p).count("]") == 0, p


@pytest.mark.parametrize("max_tokens,max_seconds", [(24, 30.0), (40, 30.0), (1000, 2.5), (60, 4.0)])
def test_split_text_properties_on_fixed_texts(max_tokens, max_seconds):
    for text in FIXED:
        _check(text, split_text(text, max_tokens=max_tokens, max_seconds=max_seconds, count_tokens=len), max_tokens, max_seconds)


def test_split_text_properties_on_a_seeded_random_mix():
    g = np.random.default_rng(5)
    words = ["a", "on", "the", "voice", "speaks", "sentence", "paragraph", "[laughter]", "[sigh]", "wonderful", "xylophones"]
    ends = ["", "", "", "", ",", ";", ":", " —", ".", "!", "?", "…"]
    seps = [" ", " ", "  ", "\n", "\t "]
    for _ in range(40):
        n = int(g.integers(1, 120))
        text = "".join(words[g.integers(len(words))] + ends[g.integers(len(ends))] + seps[g.integers(len(seps))] for _ in range(n))
        for max_tokens, max_seconds in ((16, 30.0), (33, 30.0), (500, 1.0), (90, 5.0)):   # every word (<= 11 chars + mark) fits on its own
            _check(text, split_text(text, max_tokens=max_tokens, max_seconds=max_seconds, count_tokens=len), max_tokens, max_seconds)


def test_split_text_prefers_sentences_then_clauses_then_spaces():
    text = "It fits in one piece."
    assert split_text(text, max_tokens=198, count_tokens=len) == [text]
    assert split_text("", count_tokens=len) == [] and split_text(" \n ", count_tokens=len) == []
    # two short sentences share a piece; the third no longer fits and starts the next one
    assert split_text("Hi there. How are you? I am fine, thanks.", max_tokens=24, count_tokens=len) == ["Hi there. How are you?", "I am fine, thanks."]
    # a sentence over budget is cut at its comma, not at the last space that would still fit ("... dog, and" has 48 characters)
    long_ = "The quick brown fox jumps over the lazy dog, and then it runs far away."
    assert split_text(long_, max_tokens=50, count_tokens=len) == ["The quick brown fox jumps over the lazy dog,", "and then it runs far away."]
    # no punctuation at all: whitespace
    assert split_text("aaa bbb ccc ddd eee", max_tokens=7, count_tokens=len) == ["aaa bbb", "ccc ddd", "eee"]
    # a whitespace-free run over budget is cut hard, but never inside a tag
    assert split_text("abcdefgh[laughter]ij", max_tokens=10, count_tokens=len) == ["abcdefgh", "[laughter]", "ij"]
    with pytest.raises(ValueError):
        split_text("x[laughter]", max_tokens=5, count_tokens=len)
    # the seconds budget alone (the unclamped form of estimate_duration)
    p = split_text("word " * 100, max_tokens=10 ** 6, max_seconds=2.0, count_tokens=len)
    assert all(len(x) / CHARS_PER_SECOND <= 2.0 for x in p) and " ".join(p) == " ".join(["word"] * 100)
    assert all(len(x) == 19 for x in p)      # greedy: four words (19 characters <= 23) per piece, a fifth would not fit


@pytest.mark.parametrize("case", range(len(STITCH_CASES)))
@pytest.mark.parametrize("pcm16", [False, True])
def test_numpy_stitch_equals_a_naive_per_sample_loop(case, pcm16):
    hop, batches, F, gap = STITCH_CASES[case]
    if hop > 100:   # the product-sized case would take the per-sample loop a while: same shape of case at a small hop
        hop, F, gap = 40, 15, 36
    rows, fade, S = stitch_case(hop, batches, F, gap, seed=case)
    assert len(fade) == F
    dt = np.int16 if pcm16 else np.float32
    a, b = np.full(S, 77, dt), np.full(S, 77, dt)
    for audio, lens, offs in rows:
        stitch_numpy(a, audio, lens, offs, fade)
        stitch_naive(b, audio, lens, offs, fade)
    assert np.array_equal(a, b)
    # the gaps are not touched; everything else is
    touched = np.zeros(S, bool)
    for _audio, lens, offs in rows:
        for n, o in zip(lens, offs):
            assert not touched[o:o + n].any()
            touched[o:o + n] = True
    assert (a[~touched] == 77).all() and touched.sum() == S - gap * (sum(len(r[1]) for r in rows) - 1)
    if F == 0 and not pcm16:
        for audio, lens, offs in rows:
            for r, (n, o) in enumerate(zip(lens, offs)):
                assert np.array_equal(a[o:o + n], audio[r, 0, :n])


def test_fade_table_is_the_stated_raised_cosine():
    w = fade_table(5.0)
    assert w.dtype == np.float32 and w.shape == (120,)
    want = np.array([0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / 120) for i in range(120)], np.float64).astype(np.float32)
    assert np.array_equal(w, want) and (np.diff(w) > 0).all() and 0 < w[0] < 1e-3 and 1 - 1e-3 < w[-1] < 1
    assert fade_table(0.0).shape == (0,) and fade_table(0.01).shape == (0,)
    assert np.allclose(w + w[::-1], 1.0, atol=1e-7)


@pytest.mark.parametrize("max_batch", [1, 3, 8])
def test_plan_long_groups_and_length(max_batch):
    ns = [7, 16, 11, 5, 9, 30, 2, 12, 8, 4, 6]
    groups, offsets, S = plan_long(ns, max_batch=max_batch, gap_ms=120.0)
    assert [i for g in groups for i in g] == list(range(11))
    assert all(1 <= len(g) <= max_batch for g in groups) and len(groups) == -(-11 // max_batch)
    gap = round(120.0 * 24)
    assert S == sum(HOP_SIZE * n for n in ns) + 10 * gap
    assert offsets == [sum(HOP_SIZE * n for n in ns[:i]) + i * gap for i in range(11)]
    # the plan does not depend on the grouping
    assert (offsets, S) == plan_long(ns, max_batch=8, gap_ms=120.0)[1:]
    assert plan_long(ns, max_batch, gap_ms=0.0)[2] == sum(HOP_SIZE * n for n in ns)
    assert plan_long([], max_batch)[1:] == ([], 0) and plan_long([3], max_batch, 50.0) == ([[0]], [0], 3 * HOP_SIZE)


def test_piece_seeds_are_63_bit_distinct_and_stable():
    s = [piece_seed(3, i) for i in range(24)]
    assert len(set(s)) == 24 and all(0 <= v < 2 ** 63 for v in s)
    assert s == [piece_seed(3, i) for i in range(24)] and s[0] != piece_seed(4, 0)
    assert s[1] == int(np.random.SeedSequence([3, 1]).generate_state(1, np.uint64)[0] >> 1)


def test_header_declares_the_long_form_entries():
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    for name in ("smtts_voice_expand", "smtts_randn_rows", "smtts_stitch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][1][0] is _lib.vp
    assert _lib.ABI_VERSION >= 9
