"""CPU: api._piece_rows, the one place where synthesize_long and synthesize_long_stream turn what they read back into segments, words
and Pieces, and api._to_output_samples, the one place where positions become output samples.

A hand-made text of 5 pieces behind a prefix of 2 tokens, fed group by group in two groupings, as the two calls feed it: the tables
of a group are padded to the group's longest row, so the groupings differ in everything but the result.  The expected lists are
written out below; the arithmetic is word_times': a token's frames times 3200, cut to the speech window with trim."""
import numpy as np
import pytest

from smalltts_amd import api
from smalltts_amd.phonemes import p2idx

PREFIX = [p2idx["h"], p2idx["i"]]
TEXTS = ["ab c", "d.", "e", "fg h", "i"]
TOKS = [PREFIX + [p2idx[ch] for ch in t] for t in TEXTS]
NS = [3, 4, 5, 6, 3]
OFF = (-1, -1)                                                 # a token that is not on the path
# per piece, per token (the prefix included): (first, last) frame
SPANS = [[OFF, OFF, (0, 0), (1, 1), (1, 1), (2, 2)],           # "ab" frames 0-1, "c" frame 2
         [OFF, OFF, (0, 2), (3, 3)],                           # "d" frames 0-2, "." frame 3
         [OFF, OFF, (1, 3)],                                   # "e" frames 1-3
         [OFF, OFF, (0, 1), (2, 3), (3, 3), (4, 5)],           # "fg" frames 0-3, "h" frames 4-5
         [OFF, OFF, OFF]]                                      # "i": an empty row
SEEDS = [11, 22, 33, 44, 55]
WINNER = [0, 2, 1, 0, 3]
LAT = [np.random.default_rng(i).standard_normal((n, 64)).astype(np.float32) for i, n in enumerate(NS)]
# untrimmed: the pieces 100 samples apart
OFFSETS = [0, 9700, 22600, 38700, 58000]
SEGS = [(0, 9600, 0, 1.0), (9700, 12800, 0, 1.0), (22600, 16000, 0, 1.0), (38700, 19200, 0, 1.0), (58000, 9600, 0, 1.0)]
WORDS = [(0, "word", 0, 6400), (1, "word", 6400, 9600), (2, "word", 9700, 19300), (3, "punct", 19300, 22500), (4, "word", 25800, 35400),
         (5, "word", 38700, 51500), (6, "word", 51500, 57900), (7, "word", 58000, 58000)]
# trimmed: speech windows (start, n) and gains, the windows 100 samples apart
WINDOWS = [(1000, 8000), (3200, 6400), (0, 16000), (6400, 10000), (200, 9000)]
GAINS = [1.0, 0.5, 2.0, 1.5, 0.25]
OFFSETS_T = [0, 8100, 14600, 30700, 40800]
SEGS_T = [(0, 8000, 1000, 1.0), (8100, 6400, 3200, 0.5), (14600, 16000, 0, 2.0), (30700, 10000, 6400, 1.5), (40800, 9000, 200, 0.25)]
WORDS_T = [(0, "word", 0, 5400), (1, "word", 5400, 8000), (2, "word", 8100, 14500), (3, "punct", 14500, 14500), (4, "word", 17800, 27400),
           (5, "word", 30700, 37100), (6, "word", 37100, 40700), (7, "word", 40800, 40800)]
GROUPINGS = ([[0, 1, 2], [3, 4]], [[0], [1, 2], [3, 4]])


def speak(groups, trim: bool, winners: bool, return_words: bool = True, return_pieces: bool = True):
    """Feeds the text group by group, every table padded to the group's own longest row -> the concatenated (segs, words, pieces)."""
    ep = api.Endpointing() if trim else None
    segs, words, made = [], ([] if return_words else None), ([] if return_pieces else None)
    for g in groups:
        P, N = max(len(TOKS[i]) for i in g), max(NS[i] for i in g)
        spans = np.full((len(g), P, 2), -1, np.int32)
        lat = np.full((len(g), N, 64), np.nan, np.float32)     # (nothing behind a row's frames may reach a Piece)
        for r, i in enumerate(g):
            spans[r, : len(TOKS[i])] = SPANS[i]
            lat[r, : NS[i]] = LAT[i]
        s, w, m = api._piece_rows(np.asarray([(OFFSETS_T if trim else OFFSETS)[i] for i in g], np.int64),
                                  np.asarray([WINDOWS[i] for i in g], np.int64) if trim else None,
                                  np.asarray([GAINS[i] for i in g], np.float32) if trim else None,
                                  spans if return_words else None, lat if return_pieces else None,
                                  np.asarray([WINNER[i] for i in g], np.int32) if winners else None,
                                  [TOKS[i] for i in g], [NS[i] for i in g], [SEEDS[i] for i in g], len(PREFIX), ep,
                                  return_words, return_pieces, len(words or ()))
        segs += s
        words = None if w is None else words + w
        made = None if m is None else made + m
    return segs, words, made


@pytest.mark.parametrize("winners", [False, True], ids=["own-seed", "winner-table"])
@pytest.mark.parametrize("trim", [False, True], ids=["plain", "trim"])
def test_two_groupings_give_the_literal_lists(trim, winners):
    results = [speak(g, trim, winners) for g in GROUPINGS]
    for segs, words, made in results:
        assert segs == (SEGS_T if trim else SEGS)
        assert all(type(v) is int for s in segs for v in s[:3]) and all(type(s[3]) is float for s in segs)
        assert words == (WORDS_T if trim else WORDS)
        assert [w[0] for w in words] == list(range(8))         # the index runs through the whole text
        assert len(made) == 5
        for i, p in enumerate(made):
            assert p.tokens == tuple(TOKS[i]) and p.prefix_len == 2
            assert p.latents.shape == (NS[i], 64) and np.array_equal(p.latents, LAT[i])
            assert p.seed == (api.take_seed(SEEDS[i], WINNER[i]) if winners else SEEDS[i])
            assert p.spans.shape == (len(TOKS[i]), 2) and np.array_equal(p.spans, np.asarray(SPANS[i], np.int32))
    assert results[0][:2] == results[1][:2]
    assert [p.seed for p in results[0][2]] == [p.seed for p in results[1][2]]
    assert made[0].seed == SEEDS[0] and made[3].seed == SEEDS[3]   # take 0 is the piece's own seed either way


def test_what_was_not_asked_for_is_none():
    segs, words, made = speak(GROUPINGS[0], True, False, return_words=False, return_pieces=False)
    assert segs == SEGS_T and words is None and made is None
    segs, words, made = speak(GROUPINGS[1], False, True, return_words=False)
    assert segs == SEGS and words is None and [p.spans for p in made] == [None] * 5
    assert [p.seed for p in made] == [api.take_seed(s, w) for s, w in zip(SEEDS, WINNER)]


def test_output_samples_are_the_ceiling_of_two_thirds_at_16_khz():
    dv = api.Delivery(16000)
    up = lambda s: -(-2 * s // 3)                              # ceil(2 s / 3)
    for segs24, words24 in ((SEGS, WORDS), (SEGS_T, WORDS_T)):
        segs, words = api._to_output_samples(dv, segs24, words24)
        assert segs == [(up(o), up(o + n) - up(o), up(st), g) for o, n, st, g in segs24]   # a length: the difference of its two ends
        assert words == [(i, kind, up(a), up(b)) for i, kind, a, b in words24]
    segs, words = api._to_output_samples(dv, SEGS, WORDS)
    assert segs[1] == (6467, 8533, 0, 1.0) and segs[4] == (38667, 6400, 0, 1.0)            # 9700 -> 6466.67 -> 6467; 22500 -> 15000
    assert words[3] == (3, "punct", 12867, 15000) and words[7] == (7, "word", 38667, 38667)
    assert api._to_output_samples(dv, SEGS_T, None) == ([(up(o), up(o + n) - up(o), up(st), g) for o, n, st, g in SEGS_T], None)
    assert api._to_output_samples(None, SEGS, WORDS) == (SEGS, WORDS)
    assert api._to_output_samples(api.Delivery(24000, "pcm16"), SEGS_T, WORDS_T) == (SEGS_T, WORDS_T)
