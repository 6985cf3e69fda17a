"""CPU: the host side of the streamed decode: the numpy restatement of carry_frames against its definition, the state
layout against the codec spec, the chunk plan, the C ABI's new names, the server's chunk framing and refusals with a stand-in batcher,
and the property the GPU tests lean on: the codec oracle is causal, so the whole-utterance decode is the reference for every chunk."""
import re
import socket
import threading
from http.server import ThreadingHTTPServer

import numpy as np
import pytest
import torch

from smalltts_amd import _lib
from smalltts_amd import server as S
from smalltts_amd.weights import DEFAULT_CODEC, CodecSpec, decode_state_layout
from tests.helpers import stream_ref as SR

SPECS = {   # tests/test_codec_gpu.py SPECS
    "tiny": CodecSpec(n_filters=8, ratios=(4, 2, 2), dec_depths=(2, 1, 1, 2)),
    "odd": CodecSpec(n_filters=16, ratios=(5, 3, 2), dec_depths=(1, 2, 1, 1)),
    "no_bias_no_scale_final_norm": CodecSpec(n_filters=32, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 2, 1, 1, 1, 1, 2), conv_bias=False,
                                             ffn_bias=False, layer_scale=False, final_norm=True),
}


def snr_db(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return 10 * np.log10((ref ** 2).sum() / max(((got - ref) ** 2).sum(), 1e-300))


@pytest.mark.parametrize("sizes", [(1,) * 11, (3, 8), (8, 3), (5, 6), (2, 4, 5), (9, 1, 1, 40), (7, 7)])
def test_carry_restatement_is_the_last_eight_frames_of_the_history(sizes):
    g = np.random.default_rng(sum(sizes))
    B, C = 3, 8
    state = np.zeros((B, SR.PAD, C), np.float32)           # a zero state: the start of an utterance
    history = np.zeros((B, 0, C), np.float32)
    for T in sizes:
        chunk = g.standard_normal((B, T, C)).astype(np.float32)
        img = np.concatenate([np.full((B, SR.PAD, C), np.nan, np.float32), chunk], axis=1)   # whatever the pads held is gone
        out, new = SR.carry(img, state, T)
        pad, want = SR.carry_brute(history, chunk)
        assert np.array_equal(out[:, :SR.PAD], pad) and np.array_equal(out[:, SR.PAD:], chunk)
        assert np.array_equal(new, want)
        state, history = new, np.concatenate([history, chunk], axis=1)


def test_state_layout_follows_the_spec():
    for name, spec in list(SPECS.items()) + [("default", DEFAULT_CODEC)]:
        layout, nbytes = decode_state_layout(spec)
        n = spec.n_stages
        want = ([spec.latent_dim] + [spec.dec_channels(i) for i in range(n) for _ in range(spec.dec_depths[i])]
                + [spec.dec_channels(i) for i in range(n - 1)] + [spec.dec_channels(n - 1)])
        assert [c for _, c, _ in layout] == want, name
        assert len(layout) == 1 + sum(spec.dec_depths) + (n - 1) + 1
        offs = [o for _, _, o in layout]
        assert offs == [32 * sum(want[:k]) for k in range(len(want))]          # dense, [8][C] fp32 each, 16-byte aligned
        assert all(o % 16 == 0 for o in offs)
        assert nbytes % 256 == 0 and 0 <= nbytes - 32 * sum(want) < 256
        assert layout[0][0] == "latent" and layout[-1][0] == "head" and len({k for k, _, _ in layout}) == len(layout)
    layout, nbytes = decode_state_layout(DEFAULT_CODEC)
    assert len(layout) == 34 and nbytes == 32 * (64 + 9 * 2048 + 4 * (1024 + 512 + 256 + 128 + 64) + 4 * 32) == 849920


def test_chunk_plan():
    from smalltts_amd.api import stream_chunks
    assert stream_chunks(75) == [2, 4, 8, 16, 32, 13]                           # sizes in order, then what is left
    assert stream_chunks(225) == [2, 4, 8, 16, 32, 32, 32, 32, 32, 32, 3]       # the last size repeats
    assert stream_chunks(62) == [2, 4, 8, 16, 32]                               # no empty remainder
    assert stream_chunks(1) == [1] and stream_chunks(0) == []                   # shorter than the first size: one chunk
    assert stream_chunks(7, (3,)) == [3, 3, 1] and stream_chunks(5, (8, 2)) == [5]
    for n in range(0, 300, 7):
        for cf in ((2, 4, 8, 16, 32), (1,), (5, 3)):
            got = stream_chunks(n, cf)
            assert got == SR.chunk_plan(n, cf) and sum(got) == n and all(c >= 1 for c in got)


def test_new_entries_are_in_the_header_and_the_table_at_abi_11():
    names = ("smtts_decode_state_bytes", "smtts_decode_stream_workspace_bytes", "smtts_codec_decode_stream", "smtts_test_carry_frames")
    with open(_lib.HEADER_PATH) as f:
        txt = f.read()
    assert int(re.search(r"#define\s+SMTTS_ABI_VERSION\s+(\d+)", txt).group(1)) == _lib.ABI_VERSION == 11
    syms = _lib.header_symbols()
    for n in names:
        assert n in syms and n in _lib.SIGNATURES and _lib.SIGNATURES[n][1][0] is _lib.vp      # the handle first
    assert _lib.SIGNATURES["smtts_decode_state_bytes"][0] is _lib.sz and _lib.SIGNATURES["smtts_decode_stream_workspace_bytes"][0] is _lib.sz
    assert len(_lib.SIGNATURES["smtts_codec_decode_stream"][1]) == 11 and len(_lib.SIGNATURES["smtts_test_carry_frames"][1]) == 10
    for phrase in ("ZERO slot is the start of an utterance", "at most ONCE per call", "clamps every index", "Refused with an error"):
        assert phrase in txt, phrase


# ---- the server's stream=1 against a stand-in batcher -----------------------------------------------------------------------------------
class FakeBatcher:
    """Feeds a streamed request the chunks a dispatcher would: 2, 4, ... frames of a ramp as PCM16, then None (or `fail` first)."""

    def __init__(self, fail=None):
        self.stats, self.seen, self.fail_with = {"requests": 0}, [], fail

    def submit(self, req):
        from smalltts_amd.api import stream_chunks
        self.seen.append(req)
        assert req.stream and req.chunks is not None
        if self.fail_with is not None:
            req.chunks.put(self.fail_with)
            return req.future
        for k, c in enumerate(stream_chunks(S.frames_for(req.duration))):
            req.chunks.put(np.full(S.HOP * c, k + 1, "<i2").tobytes())
        req.chunks.put(None)
        return req.future


def _serve(batcher):
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), S.make_handler(batcher, tokenizer="chars"))
    threading.Thread(target=httpd.serve_forever, kwargs={"poll_interval": 0.02}, daemon=True).start()
    return httpd


def _raw_post(port, query):
    """The answer as it is on the wire (Connection: close): (status, headers, body bytes with the chunk framing still in)"""
    wav = S.encode_wav(np.zeros(4800, np.float32))
    bd = "----t"
    body = (f"--{bd}\r\nContent-Disposition: form-data; name=\"audio\"; filename=\"r.wav\"\r\n\r\n".encode() + wav + b"\r\n"
            + f"--{bd}\r\nContent-Disposition: form-data; name=\"tokens\"\r\n\r\n1,2,3\r\n--{bd}--\r\n".encode())
    head = (f"POST /synthesize?{query} HTTP/1.1\r\nHost: x\r\nConnection: close\r\ncontent-type: multipart/form-data; boundary={bd}\r\n"
            f"content-length: {len(body)}\r\n\r\n").encode()
    with socket.create_connection(("127.0.0.1", port), timeout=10) as s:
        s.sendall(head + body)
        data = b""
        while True:
            part = s.recv(1 << 16)
            if not part:
                break
            data += part
    top, _, rest = data.partition(b"\r\n\r\n")
    lines = top.decode().split("\r\n")
    return int(lines[0].split()[1]), {k.lower(): v for k, v in (l.split(": ", 1) for l in lines[1:])}, rest


def test_server_chunk_framing_and_refusals():
    b = FakeBatcher()
    httpd = _serve(b)
    try:
        port = httpd.server_address[1]
        code, heads, raw = _raw_post(port, "duration=2.0&stream=1")              # 15 frames: chunks of 2, 4, 8, 1
        assert code == 200 and heads["transfer-encoding"] == "chunked" and "content-length" not in heads
        assert heads["content-type"] == "audio/L16; rate=24000; channels=1" and heads["x-smtts-pcm"] == "s16le"
        sizes, pcm = [], b""
        while True:                                                                 # <hex size>\r\n<data>\r\n ... 0\r\n\r\n
            n, _, raw = raw.partition(b"\r\n")
            n = int(n, 16)
            if n == 0:
                assert raw == b"\r\n"
                break
            sizes.append(n)
            pcm, raw = pcm + raw[:n], raw[n:]
            assert raw[:2] == b"\r\n"
            raw = raw[2:]
        assert sizes == [2 * S.HOP * c for c in (2, 4, 8, 1)]
        assert np.array_equal(np.frombuffer(pcm, "<i2"), np.repeat([1, 2, 3, 4], [S.HOP * c for c in (2, 4, 8, 1)]))
        assert S.http_chunk(b"ab") == b"2\r\nab\r\n" and S.http_chunk(b"") == b"0\r\n\r\n"
        seen = len(b.seen)
        for q, word in (("duration=2.0&stream=1&trim=1", b"stream"), ("duration=2.0&stream=1&align=1", b"stream"),
                        ("duration=2.0&stream=yes", b"stream"), ("duration=2.0&stream=1&trim=1&level=-20", b"stream")):
            code, heads, raw = _raw_post(port, q)
            assert code == 400 and word in raw and "transfer-encoding" not in heads, q
        assert len(b.seen) == seen                                                  # refused before they could join a batch
    finally:
        httpd.shutdown()
        httpd.server_close()
    # an error before the first chunk is an ordinary error answer
    httpd = _serve(FakeBatcher(fail=S.HttpError(500, "inference failed: boom")))
    try:
        code, heads, raw = _raw_post(httpd.server_address[1], "duration=2.0&stream=1")
        assert code == 500 and raw == b"inference failed: boom" and "transfer-encoding" not in heads
    finally:
        httpd.shutdown()
        httpd.server_close()
    # the parser alone
    assert S.parse_stream_query({}) is False and S.parse_stream_query({"stream": ["0"]}) is False
    assert S.parse_stream_query({"stream": ["true"]}) is True
    with pytest.raises(S.HttpError):
        S.parse_stream_query({"stream": ["1"]}, None, True)
    r = S.Request(None, 24000, [1], 1.0, 0)
    assert r.stream is False and r.chunks is None                                   # a plain request carries no queue


@pytest.mark.parametrize("name", ["tiny", "no_bias_no_scale_final_norm"])
def test_the_codec_oracle_is_causal(name):
    """What the GPU tests lean on: a decode of the first frames is the prefix of the whole decode (fp32 rounding: measured 2e-6
    absolute at amplitudes of about 4), while frames decoded from a fresh start are NOT the continuation (measured 1.6 dB)."""
    from oracle import codec_oracle as CO
    from oracle.dit_oracle import to_torch
    from smalltts_amd.weights import codec_decoder_param_specs, synth_state_dict
    spec = SPECS[name]
    wd = to_torch(synth_state_dict(codec_decoder_param_specs(spec), 3))
    lat = torch.randn(1, 8, 64, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        whole = CO.decode(wd, lat, spec).numpy()
        for n in (1, 3, 8):
            part = CO.decode(wd, lat[:, :n], spec).numpy()
            err = np.abs(part - whole[:, :, :spec.hop * n]).max()
            assert err <= 1e-5, (n, err)
        fresh = CO.decode(wd, lat[:, 3:], spec).numpy()
    s = snr_db(fresh, whole[:, :, spec.hop * 3:])
    assert s < 10.0, s
