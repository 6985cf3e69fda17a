"""CPU: the numpy float32 restatement of smtts_ctc_align (tests/helpers/ctc_align_ref.py), which the GPU tests compare the kernel with
bit for bit, is itself held to a brute force: every valid CTC path of 300 tiny rows enumerated in float64.  Three broken versions of the
restatement (ties the other way, the skip across equal labels, the end in the last blank only) each fail at least one case, so the
cases can tell.  Then the host logic of the alignment calls: word_times at the recogniser's hop, the mapping to codec frames, the
confidence, and every refusal that needs no device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import ctc_align_ref as R

C = 4
N_CASES = 300


def _cases(quantised: bool):
    """T in [1, 6], L in [1, 3], C = 4, log-softmax of 3 N(0, 1) logits (drawn per case in the order T, L, logits, tokens); quantised:
    rounded to multiples of 0.25, where float32 sums are exact and ties are everywhere."""
    rng = np.random.default_rng(0)
    out = []
    for _ in range(N_CASES):
        T = int(rng.integers(1, 7))
        L = int(rng.integers(1, 4))
        z = 3.0 * rng.standard_normal((T, C))
        tok = rng.integers(1, C, size=L).tolist()
        lp = z - np.log(np.exp(z - z.max(-1, keepdims=True)).sum(-1, keepdims=True)) - z.max(-1, keepdims=True)
        if quantised:
            lp = np.round(lp * 4.0) / 4.0
        out.append((lp.astype(np.float32), tok))
    return out


CONT = _cases(False)
QUANT = _cases(True)
BRUTE = {False: [R.brute_force(lp, tok) for lp, tok in CONT], True: [R.brute_force(lp, tok) for lp, tok in QUANT]}


def _disagreements(cases, brute, **wrong):
    bad = []
    for i, ((lp, tok), (want, path)) in enumerate(zip(cases, brute)):
        got = R.align(lp, lp.shape[0], tok, 0, len(tok), **wrong)
        if path is None:
            if got["state"] is not None or not np.isneginf(got["score"]):
                bad.append(i)
        elif got["state"] != path or abs(float(got["score"]) - want) > 1e-5:
            bad.append(i)
    return bad


def test_the_draw_covers_every_shape_and_both_outcomes():
    shapes = {(lp.shape[0], len(tok)) for lp, tok in CONT}
    assert shapes == {(T, L) for T in range(1, 7) for L in range(1, 4)}
    feasible = [p is not None for _s, p in BRUTE[False]]
    assert 0 < sum(feasible) < N_CASES
    for (lp, tok), ok in zip(CONT, feasible):                  # infeasible exactly when the frames do not reach: L + repeats
        need = len(tok) + sum(a == b for a, b in zip(tok, tok[1:]))
        assert ok == (lp.shape[0] >= need)


@pytest.mark.parametrize("quantised", [False, True])
def test_restatement_equals_brute_force_on_every_case(quantised):
    cases = QUANT if quantised else CONT
    assert _disagreements(cases, BRUTE[quantised]) == []
    if quantised:                                              # the sums are exact there: the score is the brute force's to the bit
        for (lp, tok), (want, path) in zip(cases, BRUTE[True]):
            if path is not None:
                assert float(R.align(lp, lp.shape[0], tok, 0, len(tok))["score"]) == want


def test_best_path_never_beats_the_sum_over_paths():
    for cases in (CONT, QUANT):
        for lp, tok in cases:
            T = lp.shape[0]
            nll = float(F.ctc_loss(torch.from_numpy(lp).double()[:, None], torch.tensor([tok]), torch.tensor([T]), torch.tensor([len(tok)]),
                                   blank=0, reduction="none", zero_infinity=False))
            score = float(R.align(lp, T, tok, 0, len(tok))["score"])
            assert score <= -nll + 1e-5, (score, nll)
            assert np.isneginf(score) == np.isposinf(nll)


@pytest.mark.parametrize("wrong,cases", [(dict(ties="move"), "quantised"), (dict(skip_equal=True), "continuous"), (dict(end="last"), "continuous")])
def test_every_broken_restatement_fails_some_case(wrong, cases):
    quantised = cases == "quantised"
    bad = _disagreements(QUANT if quantised else CONT, BRUTE[quantised], **wrong)
    print(f"{wrong}: {len(bad)} of {N_CASES} {cases} cases disagree with the brute force")
    assert bad


def test_outputs_of_a_planted_row_windows_and_clamps():
    """The outputs around the path: a window [p0, p1) inside a longer table, frames behind t_len, clamped tokens."""
    T, P = 9, 5
    lp = np.full((T + 2, C), -20.0, np.float32)
    plan = [0, 2, 2, 0, 0, 3, 3, 3, 0]                         # blank, token 1 (class 2) on 1..2, blanks, token 2 (class 3) on 5..7, blank
    for t, c in enumerate(plan):
        lp[t, c] = 0.0
    lp[T:] = np.nan                                            # behind t_len: never read
    tokens = [1, 2, 9, 1, 1]                                   # 9 is clamped to C - 1 = 3; the window is tokens [1, 3)
    r = R.align(lp, T, tokens, 1, 3)
    assert r["state"] == [0, 1, 1, 2, 2, 3, 3, 3, 4] and float(r["score"]) == 0.0
    assert r["spans"].tolist() == [[-1, -1], [1, 2], [5, 7], [-1, -1], [-1, -1]]
    assert r["tok_logp"].tolist() == [0.0] * P
    assert r["frame_tok"].tolist() == [-1, 1, 1, -1, -1, 2, 2, 2, -1, -1, -1]
    assert len(r["frame_tok"]) == T + 2 and P == len(tokens)
    for kw in (dict(t_len=0), dict(p0=3, p1=3), dict(p0=4, p1=2)):
        e = R.align(lp, kw.get("t_len", T), tokens, kw.get("p0", 1), kw.get("p1", 3))
        assert np.isneginf(e["score"]) and e["state"] is None and (e["spans"] == -1).all() and (e["frame_tok"] == -1).all()
    lp[4, 2] = np.nan                                          # a NaN in state 1 only: never greater, the best path is as it was
    e = R.align(lp, T, tokens, 1, 3)
    assert float(e["score"]) == 0.0 and e["state"] == r["state"]
    lp[4, 0] = np.nan                                          # a NaN the last blank reads stays in that state (v = delta[s] first,
    e = R.align(lp, T, tokens, 1, 3)                           # nothing is greater than it): the score is NaN, the row not aligned
    assert np.isnan(e["score"]) and e["state"] is None and (e["spans"] == -1).all() and not e["tok_logp"].any()


# ---- host logic of the alignment calls ------------------------------------------------------------------------------------------------
def test_word_times_at_the_recognisers_hop():
    from smalltts_amd.plans import CTC_HOP, HOP_SIZE, token_groups, word_times
    from smalltts_amd.phonemes import p2idx
    assert CTC_HOP == HOP_SIZE // 4 == 800
    sp, a, b = p2idx[" "], p2idx["a"], p2idx["b"]
    toks = [a, b, sp, b, p2idx["."]]
    groups = token_groups(toks)
    assert [(g[0], g[2], g[3]) for g in groups] == [("word", 0, 2), ("word", 3, 4), ("punct", 4, 5)]
    spans = np.array([[1, 2], [3, 6], [-1, -1], [9, 9], [10, 11]], np.int32)
    assert word_times(groups, spans, 12, hop=CTC_HOP) == [(0, "word", 800, 5600), (1, "word", 7200, 8000), (2, "punct", 8000, 9600)]
    # behind a prefix of two tokens, and clipped to the row's 11 frames
    pre = np.concatenate([np.full((2, 2), -1, np.int32), spans])
    assert word_times(groups, pre, 11, token0=2, hop=CTC_HOP)[-1] == (2, "punct", 8000, 8800)
    # a row that is not aligned: every group collapses
    assert word_times(groups, np.full((5, 2), -1, np.int32), 12, hop=CTC_HOP) == [(0, "word", 0, 0), (1, "word", 0, 0), (2, "punct", 0, 0)]


def test_codec_spans_is_floor_division_by_four_and_keeps_minus_one():
    from smalltts_amd.plans import codec_spans, frames_of_groups
    sp = np.array([[-1, -1], [0, 3], [4, 4], [7, 8], [11, 899]], np.int32)
    got = codec_spans(sp)
    assert got.dtype == np.int32 and got.tolist() == [[-1, -1], [0, 0], [1, 1], [1, 2], [2, 224]]
    groups = [("word", "x", 0, 2), ("word", "y", 2, 4)]
    assert frames_of_groups(groups, got, 0, 2, token0=1) == (0, 225)
    with pytest.raises(ValueError, match="not on the alignment path"):
        frames_of_groups(groups, codec_spans(np.full((5, 2), -1)), 0, 1, token0=1)
    with pytest.raises(ValueError):
        codec_spans(np.zeros((3,), np.int32))


def test_group_confidence_is_the_mean_of_tok_logp_over_span_length():
    from smalltts_amd.plans import group_confidence
    f32 = np.float32
    groups = [("word", "x", 0, 2), ("punct", ".", 2, 3)]
    spans = np.array([[-1, -1], [0, 2], [3, 3], [5, 9]], np.int32)
    tl = np.array([0.0, -0.3, -1.7, -2.5], np.float32)
    want0 = f32(f32(f32(0) + tl[1] / f32(3)) + tl[2] / f32(1)) / f32(2)
    want1 = f32(f32(0) + tl[3] / f32(5)) / f32(1)
    got = group_confidence(groups, spans, tl, token0=1)
    assert got == [float(want0), float(want1)] and all(isinstance(v, float) for v in got)
    spans[2] = (-1, -1)                                        # a token off the path: the group has no confidence
    assert group_confidence(groups, spans, tl, token0=1) == [float("-inf"), float(want1)]
    assert group_confidence(groups, np.full((4, 2), -1), np.zeros(4, np.float32), token0=1) == [float("-inf")] * 2


def test_calls_without_the_recogniser_and_bad_arguments_are_refused_before_any_device_work():
    from smalltts_amd import _lib, api
    from smalltts_amd.options import Piece

    class NoAsr:
        def has(self, part):
            return part != "asr"

    class Asr:                                                 # has the part; any device work would raise AttributeError
        device = torch.device("cpu")

        def has(self, part):
            return True

        def _dev(self, a, dtype):
            return torch.as_tensor(np.asarray(a)).to(dtype)

    tts = object.__new__(api.SmallTTS)
    tts.engine = NoAsr()
    lat = np.zeros((2, 5, 64), np.float32)
    piece = Piece([3, 4, 5], 1, lat[0], 7)
    for call in (lambda: tts.align_phonemes(lat, [[3], [4]]), lambda: tts.align_words(lat, [[3], [4]]),
                 lambda: tts.align_wav(np.zeros(24000, np.float32), 24000, [3, 4]), lambda: tts.realign([piece])):
        with pytest.raises(ValueError, match="recogniser"):
            call()
    tts.engine = Asr()
    for kw in (dict(ids=[[3]]), dict(ids=[[3], [4]], prefix_lens=[0]), dict(ids=[[3], [4]], prefix_lens=[2, 0]),
               dict(ids=[[3], [4]], prefix_lens=[-1, 0]), dict(ids=[[3] * 199, [4]]), dict(ids=[[3], [4]], lengths=[5, 6]),
               dict(ids=[[3], [4]], lengths=[5])):
        with pytest.raises(ValueError, match="align_phonemes"):
            tts.align_phonemes(lat, kw["ids"], lengths=kw.get("lengths"), prefix_lens=kw.get("prefix_lens"))
    with pytest.raises(ValueError, match="align_words"):
        tts.align_words(np.zeros((65, 5, 64), np.float32), [[3]] * 65)
    with pytest.raises(ValueError, match="align_words"):
        tts.align_words(np.zeros((1, 226, 64), np.float32), [[3]])
    for audio, sr in ((np.zeros((2, 3, 4), np.float32), 24000), (np.zeros((4, 2), np.float32), 24000), (np.zeros(0, np.float32), 24000),
                      (np.zeros(30 * 8000 + 1, np.float32), 8000), (np.zeros(100, np.float32), 0)):
        with pytest.raises(ValueError, match="align_wav"):
            tts.align_wav(audio, sr, [3, 4])
    with pytest.raises(ValueError, match="realign"):
        tts.realign([lat[0]])
    assert tts.realign([]) == []
    # the entry is declared, bound and additive
    assert "smtts_ctc_align" in _lib.SIGNATURES and "smtts_ctc_align" in _lib.header_symbols() and _lib.ABI_VERSION == 11
    assert len(_lib.SIGNATURES["smtts_ctc_align"][1]) == 15


def test_align_script_refuses_mixed_modes(capsys):
    from smalltts_amd.scripts import align
    for argv in ([], ["--wav", "a.wav", "--take", "t.npz"], ["--wav", "a.wav", "--words", "w.json"], ["--wav", "a.wav", "--text", "hi"],
                 ["--take", "t.npz"], ["--take", "t.npz", "--out-take", "o.npz", "--words", "w.json"],
                 ["--wav", "a.wav", "--text", "hi", "--words", "w.json", "--out-take", "o.npz"]):
        with pytest.raises(SystemExit) as e:
            align.main(argv)
        assert e.value.code == 2, argv
    rows = [(0, "word", "ab", 800, 5600, -0.25), (1, "punct", ".", 0, 0, float("-inf"))]
    import json
    js = json.loads(align.words_json(rows))
    assert js[0] == {"index": 0, "kind": "word", "phonemes": "ab", "start": 800, "end": 5600, "start_s": 0.0333, "end_s": 0.2333,
                     "confidence": -0.25} and js[1]["confidence"] is None
