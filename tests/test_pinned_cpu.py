"""CPU: pinned sampling and re-speaking without a GPU: the reference loop against the oracle's sampler and against itself (the pins do
something), the host helpers (frames_of_groups, splice_pins, Piece, take files), argument validation of synthesize_batch / respeak /
render_long in front of any engine call, the C entry in the signature table and the header at ABI 11."""
import re

import numpy as np
import pytest
import torch

from oracle import dit_oracle as O
from smalltts_amd import _lib, api
from tests.helpers import pinned_ref as PR


def test_reference_without_pins_is_the_oracle_sampler(dit_weights):
    case, cache, (plain, steps), _s1, _s2 = PR.tiny_refs(dit_weights)
    keep = []
    with torch.no_grad():
        want = O.sample_dmd(dit_weights, cache, case["ph_mask"], case["mask"], case["noise"], 4, keep=keep)
    assert torch.equal(plain, want) and all(torch.equal(a, b) for a, b in zip(steps, keep))


def test_reference_pins_hold_and_move_the_free_frames(dit_weights):
    """The reference is not vacuous: pinned frames come back as given after every step, and the free frames move by far more than
    the parity bar (1e-4): above 1e-2 both against the plain run (set 1: pinned to the plain run's own result) and between two sets
    of pinned values (set 2: fresh normals).  Measured on the CPU: 6.0e-2 and 9.1e-2."""
    case, _cache, (plain, _), (set1, k1), (set2, k2) = PR.tiny_refs(dit_weights)
    K = (case["pin"] & case["mask"])
    for x in [set1] + k1:
        assert torch.equal(x[K], plain[K])
    for x in [set2] + k2:
        assert torch.equal(x[K], case["fresh"][K])
    free = PR.free_valid(case)
    assert int(free.sum()) == 4 + 4          # frames [4, 8) of both rows; row 1 ends at frame 9, behind them
    e1, e2 = PR.rel(set1, plain, free), PR.rel(set2, set1, free)
    print(f"\n[pinned ref] free frames: set 1 vs plain {e1:.3e}, set 2 vs set 1 {e2:.3e}")
    assert e1 > 1e-2 and e2 > 1e-2


def test_reference_late_start(dit_weights):
    """start = k from the plain run's step k - 1 with nothing pinned continues the plain run exactly (step i draws noise[i])."""
    case, cache, (plain, steps), _s1, _s2 = PR.tiny_refs(dit_weights)
    keep = []
    with torch.no_grad():
        x = PR.sample_pinned(dit_weights, cache, case["ph_mask"], case["mask"], case["noise"], 4, steps[1], None, 2, keep=keep)
    assert len(keep) == 2 and torch.equal(x, plain) and torch.equal(keep[0], steps[2])


def test_frames_of_groups_is_word_times_mapping():
    groups = [("word", "ab", 0, 2), ("punct", ",", 2, 3), ("word", "cde", 4, 7)]
    spans = np.array([[-1, -1], [-1, -1], [0, 1], [2, 2], [3, 3], [-1, -1], [4, 4], [5, 7], [8, 9]], np.int32)   # 2 prefix tokens
    assert api.frames_of_groups(groups, spans, 0, 1, token0=2) == (0, 3)
    assert api.frames_of_groups(groups, spans, 1, 2, token0=2) == (3, 4)
    assert api.frames_of_groups(groups, spans, 0, 3, token0=2) == (0, 10)
    for g in range(3):     # the same frames word_times reports, in samples
        f0, f1 = api.frames_of_groups(groups, spans, g, g + 1, token0=2)
        assert api.word_times(groups, spans, 10, token0=2)[g][2:] == (3200 * f0, 3200 * f1)
    for bad in ((1, 1), (-1, 2), (0, 4), (2, 1)):
        with pytest.raises(ValueError):
            api.frames_of_groups(groups, spans, *bad, token0=2)
    with pytest.raises(ValueError):        # off the path
        api.frames_of_groups(groups, spans, 0, 1, token0=0)
    with pytest.raises(ValueError):        # past the table
        api.frames_of_groups(groups, spans, 2, 3, token0=3)


def test_splice_pins_copies_head_and_tail():
    lat = np.random.default_rng(0).standard_normal((10, 64)).astype(np.float32)
    x, keep = api.splice_pins(lat, 3, 6)
    assert x.shape == (10, 64) and x.dtype == np.float32 and keep.dtype == np.bool_
    assert np.array_equal(x[:3], lat[:3]) and np.array_equal(x[6:], lat[6:]) and not x[3:6].any()
    assert keep.tolist() == [True] * 3 + [False] * 3 + [True] * 4
    for m, n2 in ((1, 8), (5, 12)):
        x, keep = api.splice_pins(lat, 3, 6, m)
        assert x.shape == (n2, 64) and np.array_equal(x[:3], lat[:3]) and np.array_equal(x[3 + m:], lat[6:]) and not x[3:3 + m].any()
        assert keep.tolist() == [True] * 3 + [False] * m + [True] * 4
    x, keep = api.splice_pins(lat, 0, 10, 2)      # nothing kept
    assert x.shape == (2, 64) and not keep.any()
    for bad in ((3, 3), (6, 3), (-1, 2), (0, 11)):
        with pytest.raises(ValueError):
            api.splice_pins(lat, *bad)
    with pytest.raises(ValueError):
        api.splice_pins(lat, 3, 6, 0)
    with pytest.raises(ValueError):
        api.splice_pins(lat[:, :32], 3, 6)


def test_piece_is_immutable_and_take_files_round_trip(tmp_path):
    g = np.random.default_rng(1)
    lat = g.standard_normal((5, 64)).astype(np.float32)
    p = api.Piece([1, 2, 3], 1, lat, 2 ** 62 + 5)
    assert p.tokens == (1, 2, 3) and p.prefix_len == 1 and p.seed == 2 ** 62 + 5 and p.spans is None and np.array_equal(p.latents, lat)
    with pytest.raises(AttributeError):
        p.seed = 3
    with pytest.raises(ValueError):
        p.latents[0, 0] = 1.0
    lat[0, 0] += 1.0                       # the piece holds its own copy
    assert p.latents[0, 0] != lat[0, 0]
    for bad in (dict(latents=lat[:, :3]), dict(prefix_len=4), dict(spans=np.zeros((2, 2), np.int32))):
        with pytest.raises(ValueError):
            api.Piece(**{**dict(tokens=[1, 2, 3], prefix_len=1, latents=lat, seed=0), **bad})
    q = api.Piece([4, 5], 0, g.standard_normal((2, 64)).astype(np.float32), 7, spans=[[0, 0], [1, 1]])
    path = tmp_path / "take.npz"
    api.save_take(path, [p, q], gap_ms=80.0, trim=True, level_dbfs=-20.0)
    pieces, join = api.load_take(path)
    assert join == dict(gap_ms=80.0, fade_ms=5.0, max_batch=8, in_flight=3, trim=True, level_dbfs=-20.0)
    for a, b in zip(pieces, (p, q)):
        assert a.tokens == b.tokens and a.prefix_len == b.prefix_len and a.seed == b.seed and np.array_equal(a.latents, b.latents)
    assert pieces[0].spans is None and np.array_equal(pieces[1].spans, q.spans)
    api.save_take(path, [q])
    assert api.load_take(path)[1]["level_dbfs"] is None
    with pytest.raises(ValueError):
        api.save_take(path, [q], gap=3)


class _NoEngine:
    """Stands where the engine would: any use of it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the arguments were validated")


def _tts():
    t = api.SmallTTS.__new__(api.SmallTTS)
    t.engine, t.num_steps, t._seed, t._rng, t._replicas = _NoEngine(), 4, 0, np.random.default_rng(0), []
    return t


def test_synthesize_batch_validates_pins_before_the_engine():
    t = _tts()
    ref = [np.zeros((3, 64), np.float32)] * 2
    toks = [[1, 2], [3]]
    lat = np.zeros((5, 64), np.float32)
    keep = np.ones(5, bool)
    bad = [dict(pins=[(lat, keep)]),                                          # one entry per row
           dict(pins=[(lat, keep), (lat[:4], keep[:4])]),                     # the row's frames
           dict(pins=[(lat.astype(np.float64), keep), None]),                 # fp32
           dict(pins=[(lat, keep.astype(np.uint8)), None]),                   # bool
           dict(pins=[(lat, keep[:4]), None]),
           dict(pins=[lat, None]),                                            # a pair
           dict(pins=[(lat, keep), None], start_step=1),                      # a late start needs latents in every row
           dict(start_step=1),
           dict(pins=[(lat, keep), (lat, keep)], start_step=4),
           dict(pins=[(lat, keep), (lat, keep)], start_step=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            t.synthesize_batch(ref, toks, None, frames=[5, 5], **kw)


def test_respeak_and_render_long_validate_before_the_engine():
    t = _tts()
    lat = np.zeros((6, 64), np.float32)
    ref = np.zeros((3, 64), np.float32)
    bad = [dict(frames=(2, 4)),                                               # no reference
           dict(frames=(2, 4), ref_latents=ref, voice=object()),             # both
           dict(frames=(4, 2), ref_latents=ref), dict(frames=(0, 7), ref_latents=ref), dict(frames=3, ref_latents=ref),
           dict(frames=(2, 4), ref_latents=ref, new_frames=0),
           dict(frames=(2, 4), ref_latents=ref, new_frames=3, start_step=1),  # a late start keeps the length
           dict(frames=(2, 4), ref_latents=ref, start_step=4),
           dict(frames=(2, 4), ref_latents=ref, prefix_len=3),
           dict(frames=(2, 4), ref_latents=ref, return_alignment=True)]
    for kw in bad:
        fr = kw.pop("frames")
        with pytest.raises(ValueError):
            t.respeak([1, 2], lat, fr, **kw)
    for pieces in ([lat[:, :5]], [lat, np.zeros((0, 64), np.float32)], [np.zeros(64, np.float32)]):
        with pytest.raises(ValueError):
            t.render_long(pieces)
    with pytest.raises(ValueError):
        t.render_long([lat], max_batch=0)
    with pytest.raises(TypeError):
        t.render_long([lat], trim="yes")
    out, segs = t.render_long([], return_segments=True)      # nothing to join: no engine needed
    assert out.shape == (1, 0) and out.dtype == np.float32 and segs == []
    assert t.render_long([], pcm16=True).dtype == np.int16


def test_cli_ranges():
    from smalltts_amd.scripts import respeak as R
    assert R.parse_range("3:9", "--frames") == (3, 9)
    for bad in ("3", "3:3", "a:b", "5:2", "-1:2"):
        with pytest.raises(ValueError):
            R.parse_range(bad, "--frames")
    p = api.Piece([9, 1, 2, 3], 1, np.zeros((6, 64), np.float32), 0)
    assert R.span_frames(p, frames="2:6") == (2, 6)
    for kw in (dict(frames="2:7"), dict(groups="0:1"), dict(), dict(frames="0:1", groups="0:1")):
        with pytest.raises(ValueError):
            R.span_frames(p, **kw)


def test_entry_is_in_the_table_and_the_header_at_abi_11():
    assert _lib.ABI_VERSION == 11
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    assert re.search(r"#define\s+SMTTS_ABI_VERSION\s+(\d+)", txt).group(1) == "11"
    assert "smtts_sample_pinned" in _lib.SIGNATURES and "smtts_sample_pinned" in _lib.header_symbols()
    res, args = _lib.SIGNATURES["smtts_sample_pinned"]
    res_a, args_a = _lib.SIGNATURES["smtts_sample_align"]
    assert res is res_a and args == args_a + [_lib.vp, _lib.vp, _lib.i32]
    decl = re.search(r"int smtts_sample_pinned\(([^;]*)\);", txt).group(1)
    decl_a = re.search(r"int smtts_sample_align\(([^;]*)\);", txt).group(1)
    norm = lambda s: [" ".join(a.split()) for a in s.split(",")]
    assert norm(decl) == norm(decl_a) + ["const float* x_pin", "const uint8_t* pin", "int start_step"]
    # the header states what is verified in the words the word timings use
    assert "UNVALIDATED on trained weights" in txt and "every weight this project has run is seeded noise" in txt
