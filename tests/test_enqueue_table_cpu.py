"""What an engine call enqueues, held on the CPU: tests/host/enqueue_record.hip links the whole library (engine and C ABI included)
against recording stand-ins for the HIP runtime (tests/host/hip_record.hpp), registers the inventories written here (the DiT; a small
codec, the recogniser and the verifier), and makes the operator calls of its list under both tunings and two presets: the condition
encoder with and without its fork, denoise_step with and without a caller rope table, the samplers (plain, on a second caller stream,
N = 8, CFG, tap, pins, refused calls followed by a plain one), the DiT / encoder stage hook, the codec (decode, encode, two streamed
chunks, one stage of each half through its hook), the two scorers (with one refused call each) and their tap hook (the same, and
refused with a tap buffer one byte short).  Every kernel launch, memset, copy, event record / wait and stream / event creation is one line,
with the stream it went to.  The lines must equal tests/golden/enqueue_table.txt.gz, recorded at the commit its first line names."""
import gzip
import os
import subprocess

from smalltts_amd.weights import (CodecSpec, asr_param_specs, codec_decoder_param_specs, codec_encoder_param_specs, dit_param_specs,
                                  sv_param_specs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smalltts_amd", "csrc")


def _sections(lines):
    """[(header, body lines up to and including rc=...)] of the recorder's output"""
    out = []
    for line in lines:
        if line.startswith("== "):
            out.append((line, []))
        else:
            out[-1][1].append(line)
    return out


def _inventory(specs):
    return "".join(name + "".join(f" {d}" for d in shape) + "\n" for name, shape in specs)


# the codec, recogniser and verifier sections of every configuration; the refused ones enqueue nothing
PARTS_OK = ("codec_decode B2 T3", "codec_encode B2 one hop", "codec_decode_stream B2 T2 chunk0", "codec_decode_stream B2 T2 chunk1",
            "test_codec_stage decoder stage1 what6 T3", "test_codec_stage encoder stage6 what6 T8", "asr_logprobs B2 N5", "sv_embed B2 N6",
            "sv_embed B2 N70", "test_scorer_taps asr B2 N5", "test_scorer_taps sv B2 N6")
PARTS_REFUSED = ("asr_logprobs B2 N5 workspace one byte short", "sv_embed B2 N70 workspace one byte short",
                 "test_scorer_taps asr B2 N5 taps one byte short", "test_scorer_taps sv B2 N6 taps one byte short")


def test_every_engine_call_enqueues_the_recorded_sequence(tmp_path):
    jobs = str(min(8, os.cpu_count() or 1))
    subprocess.run(["make", "-C", CSRC, "-j", jobs, "enqueue_record"], check=True, stdout=subprocess.DEVNULL)
    inventory = tmp_path / "dit_inventory.txt"
    inventory.write_text(_inventory(dit_param_specs()))
    spec = CodecSpec(n_filters=8, ratios=(8, 5, 5, 4, 2, 2), dec_depths=(1, 1, 1, 1, 1, 1, 1))   # (the recorder hands the engine the same)
    parts = tmp_path / "parts_inventory.txt"
    parts.write_text(_inventory(codec_decoder_param_specs(spec) + codec_encoder_param_specs(spec) + asr_param_specs() + sv_param_specs()))
    got = subprocess.run([os.path.join(CSRC, "build", "enqueue_record"), str(inventory), str(parts)], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "enqueue_table.txt.gz"), "rt") as f:
        head, *want = f.read().splitlines()
    assert head.startswith("# recorded at ")
    assert len(want) > 10000
    # the table itself holds what the calls were chosen for
    for cfg in ("latency f16", "latency bf16x3", "throughput f16", "throughput bf16x3"):
        sec = [(h, b) for h, b in _sections(want) if h.endswith(f"[{cfg}]")]
        body = {h: b for h, b in sec}
        plain = [b for h, b in sec if h == f"== sample mode0 N9 [{cfg}]"]
        assert len(plain) == 4 and all(b == plain[0] for b in plain)      # a refused call leaves nothing behind for the next one
        assert plain[0][-1] == "rc=0" and len(plain[0]) > 100
        refused = [b for h, b in sec if h.startswith("== refused: ")]
        assert len(refused) == 3 and all(len(b) == 1 and b[0].startswith("rc=1 ") for b in refused)   # ... and enqueues nothing
        n9, n8 = plain[0], body[f"== sample mode0 N8 [{cfg}]"]
        assert len(n9) - len(n8) == (2 if cfg.endswith("bf16x3") else 1)   # pad8(N) != N: the V^T memset(s), once per call
        assert sum(" attn_text_mass" in l for l in body[f"== sample_align steps 10 layers a02 heads 24 [{cfg}]"]) == 3
        assert sum(" cfg_combine" in l for l in body[f"== sample mode1 cfg1 N9 [{cfg}]"]) == 2
        assert all(len(body[f"== {p} [{cfg}]"]) > 1 and body[f"== {p} [{cfg}]"][-1] == "rc=0" for p in PARTS_OK)
        assert all(len(body[f"== {p} [{cfg}]"]) == 1 and body[f"== {p} [{cfg}]"][0].startswith("rc=1 ") for p in PARTS_REFUSED)
        # the tap hook runs the product's launcher: its own workspace filled first, then the product's lines, each with one copy behind it
        for hook, entry, n in (("test_scorer_taps asr B2 N5", "asr_logprobs B2 N5", 44), ("test_scorer_taps sv B2 N6", "sv_embed B2 N6", 23)):
            tapped, product = body[f"== {hook} [{cfg}]"], body[f"== {entry} [{cfg}]"]
            assert tapped[0] == "main memset whole" and len(product) == n + 1
            assert tapped[1::2] == product and all(l.startswith("main memcpy ") and l.endswith(" d2d") for l in tapped[2:-1:2])
    lat = {h: b for h, b in _sections(want) if h.endswith("[latency f16]")}
    assert lat["== cond_encode B2 R3 P5 [latency f16]"][:5] == ["create side0", "create ev0", "create ev1", "main record ev0", "side0 wait ev0"]
    assert not any(l.startswith(("side", "create")) for l in lat["== cond_encode B2 R3 P0 [latency f16]"])
    main2 = lat["== sample mode0 N9 on main2 [latency f16]"]
    assert "create side1" in main2 and not any(l.startswith(("main ", "side0 ")) for l in main2)
    assert any(l == "main wait ev1" for l in lat["== sample mode0 N9 [latency f16]"])
    diff = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not diff, f"{len(diff)} lines differ, first: {diff[0]}"
    assert len(got) == len(want)
