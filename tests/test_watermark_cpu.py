"""Watermark without a GPU: the restatement against itself (chunked == whole, bit for bit), the statistics the scheme
promises (conditions the restatement alone meets, fixed seeds), the ABI bookkeeping and the host-side refusals."""
import os

import numpy as np
import pytest

from smalltts_amd import _lib
from tests.helpers import watermark_ref as W

KEY = 0x5EEDC0DE12345678
STRENGTH = 0.02


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _signal(n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.3 * np.sin(0.05 * t) * (1 + 0.5 * np.sin(0.003 * t)) + 0.02 * rng.standard_normal(n)).astype(np.float32)


def _chunkings(n):
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.choice(np.arange(1, n), 9, replace=False))
    return {
        "ones": [1] * n,
        "63/64/65": [63, 64, 65] * (n // 192) + [n - 192 * (n // 192)],
        "127/128": [127, 128] * (n // 255) + [n - 255 * (n // 255)],
        "an empty chunk": [100, 0, 64, 0, n - 164],
        "random": list(np.diff(np.concatenate([[0], cuts, [n]]))),
    }


# ---- 1. the restatement, chunked against whole ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ones", "63/64/65", "127/128", "an empty chunk", "random"])
def test_chunked_restatement_is_the_whole_restatement(name):
    n = 1000
    x = _signal(n)
    whole = W.embed(x, KEY, STRENGTH)
    sizes = _chunkings(n)[name]
    assert sum(sizes) == n
    st, pos, outs = W.Stream(KEY, STRENGTH), 0, []
    for c in sizes:
        outs.append(st.push(x[pos: pos + c]))
        pos += c
        want = np.concatenate([np.zeros(W.HIST, np.float32), x[:pos]])[-W.HIST:]
        assert np.array_equal(_bits(st.hist), _bits(want)) and st.n == pos          # .hist after every push
    assert np.array_equal(_bits(np.concatenate(outs)), _bits(whole))


def test_first_block_silence_and_zero_strength():
    x = _signal(640)
    y = W.embed(x, KEY, STRENGTH)
    assert np.array_equal(_bits(y[:64]), _bits(x[:64]))                              # the first block is never marked
    assert not np.array_equal(y[64:], x[64:])
    z = np.zeros(640, np.float32)
    assert np.array_equal(_bits(W.embed(z, KEY, STRENGTH)), _bits(z))               # silence stays exact silence
    gap = x.copy()
    gap[128:320] = 0.0                                                               # ... also inside a signal: blocks 3 and 4 follow silence
    assert np.array_equal(_bits(W.embed(gap, KEY, STRENGTH)[192:320]), _bits(gap[192:320]))
    assert np.array_equal(W.embed(x, KEY, 0.0), x)                                   # strength 0: the identity
    # the mark is +- A, A = strength * the RMS of the block in front (one float32 chain)
    a = np.abs(y.astype(np.float64) - x.astype(np.float64))[64:128]
    rms = np.sqrt(np.mean(x[:64].astype(np.float64) ** 2))
    assert np.allclose(a, STRENGTH * rms, rtol=1e-4)


def test_chips_are_philox_words_and_balanced():
    from oracle import philox
    # 2^33 + 5: a position past 32 bits; 2^39 + 5: the counter i >> 7 itself passes 32 bits there, its high word is 1
    for i0 in (2 ** 33 + 5, 2 ** 39 + 5):
        c = W.chips(i0, 300, KEY)
        for i in (i0, i0 + 26, i0 + 27, i0 + 122, i0 + 123, i0 + 299):              # across a word and a group
            g = i >> 7
            ctr = np.array([[g & 0xFFFFFFFF, g >> 32, 0x574D4B31, 0]], np.uint32)
            w = philox.philox4x32_10(ctr, KEY)[0]
            bit = (int(w[(i >> 5) & 3]) >> (i & 31)) & 1
            assert c[i - i0] == (1 if bit else -1)
    assert ((2 ** 39 + 5) >> 7) >> 32 == 1
    assert not np.array_equal(W.chips(2 ** 39 + 5, 300, KEY), W.chips(5, 300, KEY))  # (the low words agree, the high word differs)
    big = W.chips(0, 1 << 16, KEY).astype(np.int64)
    assert abs(big.sum()) < 5 * 256 and not np.array_equal(big, W.chips(0, 1 << 16, KEY + 1))


@pytest.mark.parametrize("start", [2 ** 33 + 5, 2 ** 39 + 5])
def test_n_before_past_32_bits(start):
    n = 700
    x = _signal(n, 3)
    whole = W.Stream(KEY, STRENGTH, start=start).push(x)
    st = W.Stream(KEY, STRENGTH, start=start)
    parts = [st.push(x[a: a + 97]) for a in range(0, n, 97)]
    assert np.array_equal(_bits(np.concatenate(parts)), _bits(whole))
    assert not np.array_equal(whole, W.embed(x, KEY, STRENGTH))                      # other chips than at position 0
    # block boundaries follow the absolute position: start = 5 mod 64, so x[0 .. 59) belongs to a block whose predecessor is the
    # (zero) slot and stays unmarked, the next sample is marked
    assert np.array_equal(_bits(whole[:59]), _bits(x[:59])) and whole[59] != x[59]


# ---- 2. the statistics, fixed seeds --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def speech():
    x = W.speechlike(10.0, seed=0)
    y = W.pcm16_round(W.embed(x, KEY, STRENGTH))
    return x, y


def test_marked_pcm16_is_detected_with_twice_the_threshold(speech):
    x, y = speech
    mark_db = 10 * np.log10(np.mean((W.embed(x, KEY, STRENGTH).astype(np.float64) - x) ** 2) / np.mean(x.astype(np.float64) ** 2))
    d = W.detect(y, KEY, 0, 1)
    print(f"10 s, PCM16, strength {STRENGTH}: mark {mark_db:.1f} dB, z(0) = {d['z'][0]:.1f}")
    assert d["z"][0] >= 12.0
    d2 = W.detect(y[:48000], KEY, 0, 1)
    print(f"2 s prefix: z(0) = {d2['z'][0]:.1f}")
    assert d2["z"][0] >= 12.0


def test_cropped_audio_is_found_at_its_offset(speech):
    _x, y = speech
    crop = 1003                                                                      # no multiple of 64
    d = W.detect(y[crop:], KEY, 0, 1100)
    print(f"cropped by {crop}: best offset {d['best_off']}, z = {d['best_z']:.1f}")
    assert d["best_off"] == crop and d["best_z"] >= 12.0


def test_unmarked_and_wrong_key_stay_below_5(speech):
    x, y = speech
    a = W.detect(W.pcm16_round(x), KEY, 0, 256)["z"]
    b = W.detect(y, KEY ^ 0xFFFF, 0, 256)["z"]
    print(f"unmarked: max |z| = {np.abs(a).max():.2f}; another key: max |z| = {np.abs(b).max():.2f}")
    assert np.abs(a).max() < 5.0 and np.abs(b).max() < 5.0


# ---- 3. ABI bookkeeping ------------------------------------------------------------------------------------------------------------------
ENTRIES = ("smtts_watermark_state_bytes", "smtts_watermark", "smtts_watermark_detect_workspace_bytes", "smtts_watermark_detect")


def test_the_c_abi_table_has_the_entries():
    assert set(ENTRIES) <= set(_lib.header_symbols()) and set(ENTRIES) <= set(_lib.SIGNATURES) and _lib.ABI_VERSION == 11
    assert len(_lib.SIGNATURES["smtts_watermark"][1]) == 11 and len(_lib.SIGNATURES["smtts_watermark_detect"][1]) == 16
    assert _lib.SIGNATURES["smtts_watermark_state_bytes"] == (_lib.sz, [_lib.vp])
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmalltts_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert lib.smtts_watermark_state_bytes(None) == 0 and b"smtts_watermark_state_bytes" in lib.smtts_last_error(None)
    assert lib.smtts_watermark(None, None, None, 1, 1, None, 0, 0.0, None, 0, None) == 1
    assert b"smtts_watermark" in lib.smtts_last_error(None)
    assert lib.smtts_watermark_detect_workspace_bytes(None, 1, 1) == 0
    assert lib.smtts_watermark_detect(None, None, None, 1, 1, None, 0, 0, 1, None, 0, None, None, None, None, None) == 1
    assert b"smtts_watermark_detect" in lib.smtts_last_error(None)


# ---- 4. host-side refusals ---------------------------------------------------------------------------------------------------------------
def test_watermark_class():
    from smalltts_amd.api import Watermark, as_watermark
    w = Watermark(7)
    assert (w.key, w.strength) == (7, 0.02) and repr(w) == "Watermark(key=7, strength=0.02)"
    assert w == Watermark(7, 0.02) and w != Watermark(8) and w != Watermark(7, 0.03) and hash(w) == hash(Watermark(7))
    assert Watermark(2 ** 64 - 1, 1.0).key == 2 ** 64 - 1 and Watermark(0, 0).strength == 0.0
    with pytest.raises(AttributeError):
        w.key = 1
    with pytest.raises((AttributeError, TypeError)):
        del w.strength
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            Watermark(bad)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            Watermark(1, bad)
    for bad in ("7", 7.0, True, None):
        with pytest.raises(TypeError):
            Watermark(bad)
    with pytest.raises(TypeError):
        Watermark(1, "0.02")
    assert as_watermark(None) is None and as_watermark(w) is w and as_watermark(9) == Watermark(9)
    assert as_watermark((9, 0.1)) == Watermark(9, 0.1)
    for bad in ("9", 9.0, True, (9,)):
        with pytest.raises(TypeError):
            as_watermark(bad)


def test_rate_encoding_trim_and_pcm16_are_refused_before_any_work():
    from smalltts_amd.api import Decoder, DecodeStream, Delivery, SmallTTS, marked_delivery
    assert marked_delivery("x", None, None) == (None, None)
    assert marked_delivery("x", 5, None)[1] == Delivery(24000, "f32")                # without deliver=
    assert marked_delivery("x", 5, Delivery(24000, "pcm16"))[1] == Delivery(24000, "pcm16")
    tts = object.__new__(SmallTTS)                                                   # no engine: the refusals come first
    dec = object.__new__(Decoder)
    dec.engine = None
    for dv in (8000, 48000, (24000, "mulaw"), (24000, "alaw"), (16000, "pcm16")):
        for call in (lambda: tts.synthesize_batch(None, [[1]], [1.0], deliver=dv, watermark=5),
                     lambda: tts.synthesize_long(None, "x", deliver=dv, watermark=5),
                     lambda: tts.synthesize_long_stream(None, "x", deliver=dv, watermark=5),
                     lambda: tts.synthesize_stream(None, [1], 1.0, deliver=dv, watermark=5),
                     lambda: DecodeStream(None, 1, dv, 5),
                     lambda: dec.open_stream(1, dv, 5)):
            with pytest.raises(ValueError, match="watermark= needs 24000 Hz"):
                call()
    with pytest.raises(ValueError, match="trim="):
        tts.synthesize_batch(None, [[1]], [1.0], watermark=5, trim=True)
    for call in (lambda: tts.synthesize_long(None, "x", watermark=5, pcm16=True),
                 lambda: tts.synthesize_long_stream(None, "x", watermark=5, pcm16=True),
                 lambda: tts.synthesize_stream(None, [1], 1.0, watermark=5, pcm16=True)):
        with pytest.raises(ValueError, match="pcm16=True"):
            call()
    with pytest.raises(TypeError):
        tts.synthesize_stream(None, [1], 1.0, watermark="5")


def test_detect_cli_arguments(tmp_path, capsys):
    from smalltts_amd.audio import write_wav_pcm16
    from smalltts_amd.scripts import detect as D
    a = D.parse_args(["--wav", "f.wav", "--key", "0x10"])
    assert (a.key, a.max_offset, a.threshold) == (16, 0, 6.0)
    a = D.parse_args(["--wav", "f.wav", "--key", "12", "--max-offset", "5000", "--threshold", "8"])
    assert (a.key, a.max_offset, a.threshold) == (12, 5000, 8.0)
    for bad in (["--wav", "f.wav"], ["--key", "1"], ["--wav", "f.wav", "--key", "-1"], ["--wav", "f.wav", "--key", "x"],
                ["--wav", "f.wav", "--key", "1", "--max-offset", "-1"], ["--wav", "f.wav", "--key", str(2 ** 64)]):
        with pytest.raises(SystemExit) as e:
            D.parse_args(bad)
        assert e.value.code == 2
    capsys.readouterr()
    # a PCM16 file comes back as the int16 it stores; another rate is refused in front of the engine
    s = (np.arange(-500, 500) * 60).astype(np.int16)
    p = str(tmp_path / "a.wav")
    write_wav_pcm16(p, s.astype(np.float32) / np.float32(32767.0), 24_000)
    x, sr = D.load(p)
    assert sr == 24_000 and x.dtype == np.int16 and np.array_equal(x, s)
    q = str(tmp_path / "b.wav")
    write_wav_pcm16(q, np.zeros(100, np.float32), 16_000)
    with pytest.raises(SystemExit, match="24000 Hz only"):
        D.main(["--wav", q, "--key", "1"])


def test_cli_watermark_flags():
    import argparse
    from smalltts_amd.api import Delivery, Watermark
    from smalltts_amd.scripts import _common as C
    ap = argparse.ArgumentParser()
    C.add_delivery_args(ap)
    C.add_watermark_args(ap)
    parse = lambda argv: (lambda a: C.watermark_for(ap, a, C.delivery_for(a)))(ap.parse_args(argv))
    assert parse([]) == (None, None)
    assert parse(["--watermark", "0x2a"]) == (Watermark(42), Delivery(24000, "pcm16"))
    assert parse(["--watermark", "42", "--watermark-strength", "0.05", "--encoding", "pcm16"]) == (Watermark(42, 0.05), Delivery(24000, "pcm16"))
    for bad in (["--watermark-strength", "0.05"], ["--watermark", "1", "--rate", "8000"], ["--watermark", "1", "--encoding", "mulaw"],
                ["--watermark", "1", "--watermark-strength", "2"], ["--watermark", "-3"]):
        with pytest.raises(SystemExit):
            parse(bad)
