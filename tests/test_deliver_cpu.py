"""CPU: the host side of delivery: the emission rule against its definition, the numpy restatement of smtts_deliver
(tests/helpers/deliver_ref.py) chunked against whole, its G.711 encoders against audioop's codes for every int16 value
(tests/golden/g711_codes.npz, written by tests/golden/make_g711_codes.py), the output banks, the WAV writer and reader, the server's
query parsing, the Delivery class and the C ABI's table."""
import itertools
import math
import os

import numpy as np
import pytest

from smalltts_amd import _lib
from smalltts_amd import audio as A
from tests.conftest import golden
from tests.helpers import deliver_ref as R

GEOMETRIES = [(1, 3, 4), (1, 3, 10), (2, 3, 5), (2, 1, 4), (147, 80, 4), (4, 3, 4), (1, 3, 0), (3, 7, 1)]   # (up, down, width)


@pytest.mark.parametrize("up,down,width", GEOMETRIES)
def test_deliver_counts_is_the_emission_rule_by_brute_force(up, down, width):
    """A frame is emitted by the first call at whose end all its klen inputs have arrived; the last call emits the rest."""
    for nb, ln, last in itertools.product(range(0, 40), (0, 1, 2, 3, 7, 11, 29), (False, True)):
        want = R.count_brute(nb, ln, last, up, down, width)
        assert A.deliver_counts(nb, ln, last, up, down, width) == want == R.count(nb, ln, last, up, down, width), (nb, ln, last)
    assert A.deliver_counts([0, 5], [9, 9], [False, True], up, down, width) == [A.deliver_counts(0, 9, False, up, down, width),
                                                                               A.deliver_counts(5, 9, True, up, down, width)]
    # every chunking of a stream hands out ceil(up * n / down) samples in all, none twice; no chunk exceeds deliver_max_count
    for split in ([50], [1] * 50, [3, 10, 11, 26], [9, 1, 40], [50, 0]):
        pos, total = 0, 0
        for k, c in enumerate(split):
            got = A.deliver_counts(pos, c, k == len(split) - 1, up, down, width)
            assert 0 <= got <= A.deliver_max_count(max(c, 1), up, down, width, True)
            total, pos = total + got, pos + c
        assert total == -(-up * 50 // down)
    assert A.deliver_max_count(64, up, down, width, False) == -(-up * 64 // down)
    with pytest.raises(ValueError):
        A.deliver_counts(-1, 3, True, up, down, width)


@pytest.mark.parametrize("rate,zeros,n", [(8000, 3, 50), (8000, 1, 50), (44100, 3, 257), (16000, 3, 50), (48000, 3, 50)])
def test_chunked_restatement_is_the_whole_restatement(rate, zeros, n):
    up, down = A.deliver_ratio(rate)
    bank, width = A._sinc_kernel(down, up, zeros)
    x = np.random.default_rng(n).uniform(-0.5, 0.5, n).astype(np.float32)
    whole, mag = R.deliver_whole(x, bank, down, width)
    assert whole.size == math.ceil(up * n / down) == A.resample_hq(x, 24000, rate).size or zeros != 1024
    for split in ([n], [1] * n, [3, 10, 11, n - 24], [9, 1, n - 10], [n, 0]):
        st, pos, parts = R.Stream(bank, down, width), 0, []
        for k, c in enumerate(split):
            y, _m = st.push(x[pos:pos + c], k == len(split) - 1)
            parts.append(y)
            pos += c
            want_hist = np.concatenate([np.zeros(bank.shape[1] - 1, np.float32), x[:pos]])[-(bank.shape[1] - 1):]
            assert np.array_equal(st.hist, want_hist)
        assert np.array_equal(np.concatenate(parts), whole), split
    # the definition agrees with the input side's resampler on the same bank (fp32 matmul there, fp64 here)
    big, w1024 = A._sinc_kernel(down, up)
    if up * big.shape[1] < 1 << 20:
        y64, m = R.deliver_whole(x, big, down, w1024)
        assert np.abs(A.resample_hq(x, 24000, rate) - y64).max() <= 1e-5


def test_g711_encoders_are_audioops_for_every_int16():
    codes = golden("g711_codes.npz")
    s = np.arange(-32768, 32768).astype(np.int16)
    assert codes["mulaw"].shape == codes["alaw"].shape == (65536,) and codes["mulaw"].dtype == np.uint8
    assert np.array_equal(R.mulaw(s), codes["mulaw"]) and np.array_equal(R.alaw(s), codes["alaw"])
    known = {0: "ffd5", 1: "ffd5", -1: "7e55", 4: "fed5", -4: "7e55", 100: "f2d3", -100: "7253", 1000: "cefa", -1000: "4e7a",
             32635: "80aa", 32767: "80aa", -32768: "002a"}
    for v, want in known.items():
        assert bytes([codes["mulaw"][v + 32768], codes["alaw"][v + 32768]]).hex() == want, v
    try:
        import audioop
    except ImportError:
        return
    pcm = s.astype("<i2").tobytes()
    assert np.array_equal(np.frombuffer(audioop.lin2ulaw(pcm, 2), np.uint8), R.mulaw(s))
    assert np.array_equal(np.frombuffer(audioop.lin2alaw(pcm, 2), np.uint8), R.alaw(s))
    assert np.array_equal(np.frombuffer(audioop.ulaw2lin(codes["mulaw"].tobytes(), 2), "<i2"), A.g711_decode(codes["mulaw"], "mulaw"))
    assert np.array_equal(np.frombuffer(audioop.alaw2lin(codes["alaw"].tobytes(), 2), "<i2"), A.g711_decode(codes["alaw"], "alaw"))


@pytest.mark.parametrize("law", ["mulaw", "alaw"])
def test_g711_decode_of_encode_is_monotone_and_within_the_segments_step(law):
    s = np.arange(-32768, 32768)
    enc, dec, shift = (R.mulaw, R.mulaw_decode, 2) if law == "mulaw" else (R.alaw, R.alaw_decode, 3)
    c = enc(s.astype(np.int16))
    d = dec(c)
    assert np.array_equal(d, A.g711_decode(c, law))
    assert (np.diff(d) >= 0).all()
    # a segment's quantisation step: 2^(seg + 1) (mu-law, 14-bit) / 2^max(seg, 1) (A-law, 13-bit) in the encoder's domain, times the
    # 2 / 3 bits the encoder drops; the decoder answers inside the cell, so the error stays below one step (clipping excepted)
    seg = ((c.astype(np.int64) ^ (0xFF if law == "mulaw" else 0x55)) >> 4) & 7
    step = (1 << (seg + 1) if law == "mulaw" else 1 << np.maximum(seg, 1)) << shift
    inside = np.abs(s) <= (32635 if law == "mulaw" else 32767)
    assert (np.abs(d - s)[inside] <= step[inside]).all()
    assert (np.abs(d - s)[~inside] <= 32768 - 32124).all()
    assert len(np.unique(c)) == (255 if law == "mulaw" else 256)   # mu-law: +0 and -0 share no code, but 0x7f is the one unused


def test_output_banks():
    for orig, new in ((3, 2), (441, 240), (2, 1)):   # today's bank, restated from the published algorithm with the width fixed at 1024
        k, w = A._sinc_kernel(orig, new, zeros=1024)
        k0, w0 = A._sinc_kernel(orig, new)
        base = min(orig, new) * A.RESAMPLE_ROLLOFF
        width = int(math.ceil(1024 * orig / base))
        idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
        t = np.clip((np.arange(0, -new, -1, dtype=np.float64)[:, None] / new + idx) * base, -1024, 1024)
        window = np.i0(A.RESAMPLE_BETA * np.sqrt(1.0 - (t / 1024) ** 2)) / np.i0(A.RESAMPLE_BETA)
        t = t * math.pi
        with np.errstate(invalid="ignore", divide="ignore"):
            today = (np.where(t == 0.0, 1.0, np.sin(t) / t) * window * (base / orig)).astype(np.float32)
        assert w == w0 == width and np.array_equal(k.view(np.uint32), today.view(np.uint32)) and np.array_equal(k0.view(np.uint32), today.view(np.uint32))
    assert A.DELIVER_ZEROS == 64
    geo = {8000: (1, 3, 205, 413), 11025: (147, 320, 149, 618), 16000: (2, 3, 103, 209), 22050: (147, 160, 75, 310),
           32000: (4, 3, 69, 141), 44100: (147, 80, 69, 218), 48000: (2, 1, 69, 139)}
    for rate, (up, down, width, klen) in geo.items():
        assert A.deliver_ratio(rate) == (up, down)
        k, w = A._sinc_kernel(down, up, A.DELIVER_ZEROS)
        assert w == width and k.shape == (up, klen) and klen == 2 * width + down
        assert abs(float(k.sum()) / up - 1.0) < 2e-3          # unity gain at DC, every phase together
    assert A.deliver_ratio(24000) == (1, 1)
    with pytest.raises(ValueError):
        A.deliver_ratio(12000)
    k3, w3 = A._sinc_kernel(80, 147, 3)
    assert (w3, k3.shape) == (4, (147, 88))


@pytest.mark.parametrize("encoding,tag,bits", [("pcm16", 1, 16), ("mulaw", 7, 8), ("alaw", 6, 8), ("f32", 3, 32)])
@pytest.mark.parametrize("n", [0, 1, 800, 801])
def test_wav_headers_read_back(tmp_path, encoding, tag, bits, n):
    import struct
    pcm = (np.random.default_rng(n).integers(-20000, 20000, n)).astype(np.int16)
    data = {"pcm16": pcm, "mulaw": R.mulaw(pcm), "alaw": R.alaw(pcm), "f32": (pcm / 32768.0).astype(np.float32)}[encoding]
    path = str(tmp_path / "a.wav")
    A.write_wav(path, data, 8000, encoding)
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8 and len(raw) % 2 == 0
    fmt = raw.index(b"fmt ")
    ftag, ch, sr, bps, blk, fbits = struct.unpack("<HHIIHH", raw[fmt + 8:fmt + 24])
    assert (ftag, ch, sr, bps, blk, fbits) == (tag, 1, 8000, 8000 * bits // 8, bits // 8, bits)
    if tag != 1:
        fact = raw.index(b"fact")
        assert struct.unpack("<II", raw[fact + 4:fact + 12]) == (4, n)
    assert raw == A.wav_bytes(data, 8000, encoding)
    y, rate = A.read_wav(path)
    assert rate == 8000 and y.shape == (n,)
    want = {"pcm16": pcm / 32768.0, "f32": pcm / 32768.0, "mulaw": R.mulaw_decode(R.mulaw(pcm)) / 32768.0,
            "alaw": R.alaw_decode(R.alaw(pcm)) / 32768.0}[encoding]
    assert np.array_equal(y, want.astype(np.float32))
    with pytest.raises(ValueError):
        A.wav_bytes(data.astype(np.float64), 8000, encoding)
    with pytest.raises(ValueError):
        A.wav_bytes(data, 8000, "s16")


def test_write_wav_pcm16_is_unchanged(tmp_path):
    x = np.linspace(-1.2, 1.2, 101, dtype=np.float32)
    A.write_wav_pcm16(str(tmp_path / "a.wav"), x)
    raw = open(str(tmp_path / "a.wav"), "rb").read()
    assert len(raw) == 44 + 202 and raw[20:22] == b"\x01\x00"
    assert raw == A.wav_bytes(np.round(np.clip(x, -1, 1) * 32767.0).astype(np.int16), 24000, "pcm16")


def test_server_query_parsing():
    from smalltts_amd import server as S
    from smalltts_amd.api import Delivery, Endpointing
    assert S.parse_deliver_query({}) is None and S.parse_deliver_query({"duration": ["2"], "stream": ["1"]}) is None
    assert S.parse_deliver_query({"rate": ["8000"], "encoding": ["mulaw"]}) == Delivery(8000, "mulaw")
    assert S.parse_deliver_query({"rate": [" 44100 "]}) == Delivery(44100, "pcm16")
    assert S.parse_deliver_query({"encoding": ["ALAW"]}) == Delivery(24000, "alaw")
    assert S.parse_deliver_query({"rate": ["16000"]}, Endpointing()) == Delivery(16000, "pcm16")
    for q in ({"rate": ["12000"]}, {"rate": ["8k"]}, {"rate": [""]}, {"rate": ["-8000"]}, {"rate": ["8000.0"]}, {"encoding": ["f32"]},
              {"encoding": ["ulaw"]}, {"encoding": [""]}, {"rate": ["8000"], "encoding": ["mp3"]}):
        with pytest.raises(S.HttpError) as e:
            S.parse_deliver_query(q)
        assert e.value.code == 400, q
    with pytest.raises(S.HttpError) as e:
        S.parse_deliver_query({"rate": ["8000"]}, Endpointing(level_dbfs=-20.0))
    assert e.value.code == 400 and "level" in e.value.msg
    r = S.Request(None, 24000, [1], 1.0, 0, deliver=Delivery(8000, "alaw"))
    assert r.deliver == Delivery(8000, "alaw") and S.Request(None, 24000, [1], 1.0, 0).deliver is None
    assert S.STREAM_TYPES["mulaw"][0].format(rate=8000) == "audio/PCMU; rate=8000" and S.STREAM_TYPES["alaw"][1] == "alaw"
    assert S.STREAM_TYPES["pcm16"] == ("audio/L16; rate={rate}; channels=1", "s16le")


def test_delivery_class():
    from smalltts_amd.api import Delivery, as_delivery
    d = Delivery()
    assert (d.rate, d.encoding, d.ratio, d.dtype) == (24000, "f32", (1, 1), np.float32) and d.samples(3200) == 3200
    e = Delivery(8000, "mulaw")
    assert e == Delivery(8000, "mulaw") and hash(e) == hash(Delivery(8000, "mulaw")) and e != d and e != (8000, "mulaw")
    assert repr(e) == "Delivery(rate=8000, encoding='mulaw')" and e.ratio == (1, 3) and e.dtype == np.uint8
    assert e.samples(3200) == 1067 and Delivery(44100).samples(3200 * 15) == 88200 and Delivery(48000, "pcm16").dtype == np.int16
    with pytest.raises(AttributeError):
        e.rate = 16000
    for bad in (12000, 0, -8000):
        with pytest.raises(ValueError):
            Delivery(bad)
    with pytest.raises(ValueError):
        Delivery(8000, "ulaw")
    for bad in (8000.0, "8000", True, None):
        with pytest.raises(TypeError):
            Delivery(bad)
    assert as_delivery(None) is None and as_delivery(e) is e and as_delivery(16000) == Delivery(16000)
    assert as_delivery((8000, "alaw")) == Delivery(8000, "alaw")
    for bad in ("8000", 8000.0, True, (8000,)):
        with pytest.raises(TypeError):
            as_delivery(bad)


def test_the_c_abi_table_has_the_entries():
    assert len(_lib.SIGNATURES["smtts_deliver"][1]) == 16 and _lib.SIGNATURES["smtts_deliver_state_bytes"] == (_lib.sz, [_lib.vp, _lib.i32])
    assert {"smtts_deliver", "smtts_deliver_state_bytes"} <= set(_lib.header_symbols()) and _lib.ABI_VERSION == 11
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libsmalltts_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    assert lib.smtts_deliver_state_bytes(None, 413) == 0 and b"smtts_deliver_state_bytes" in lib.smtts_last_error(None)
    assert lib.smtts_deliver(None, None, None, 1, 1, None, None, 1, 1, 0, 0, None, 0, 0, None, 1) == 1
    assert b"smtts_deliver" in lib.smtts_last_error(None)
