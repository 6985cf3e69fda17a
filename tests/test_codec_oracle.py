"""CPU: structural checks of the build-defined codec oracle (parity vs the reference is unpinned —
see oracle/codec_oracle.py). Pins what the reference does pin: I/O shapes and hop = 3200."""
import numpy as np
import torch

from oracle import codec_oracle as CO
from oracle.dit_oracle import to_torch
from smalltts_amd.weights import (DEFAULT_CODEC, CodecSpec, codec_decoder_param_specs, codec_encoder_param_specs,
                                  synth_state_dict)

SMALL = CodecSpec(latent_dim=64, n_filters=8, ratios=(4, 2, 2), dec_depths=(2, 1, 1, 2))


def test_default_spec_matches_reference_contract():
    assert DEFAULT_CODEC.hop == 3200 and DEFAULT_CODEC.latent_dim == 64  # infer/onnx.py:11-12
    n = sum(int(np.prod(s)) for _, s in codec_decoder_param_specs())
    assert 3.3e8 < n < 3.6e8  # ~340 M parameters per codec half


def test_decode_shape_and_causality():
    w = to_torch(synth_state_dict(codec_decoder_param_specs(SMALL), 1))
    lat = torch.randn(2, 6, 64)
    with torch.no_grad():
        a = CO.decode(w, lat, SMALL)
        lat2 = lat.clone(); lat2[:, 4:] += 1.0
        b = CO.decode(w, lat2, SMALL)
    assert a.shape == (2, 1, SMALL.hop * 6)
    cut = 4 * SMALL.hop
    assert torch.equal(a[..., :cut], b[..., :cut]) and not torch.equal(a[..., cut:], b[..., cut:])


def test_encode_shape_and_causality():
    w = to_torch(synth_state_dict(codec_encoder_param_specs(SMALL), 1))
    au = torch.randn(2, 1, SMALL.hop * 5 + 3)
    with torch.no_grad():
        a = CO.encode(w, au, SMALL)
        au2 = au.clone(); au2[..., 3 * SMALL.hop:] += 0.5
        b = CO.encode(w, au2, SMALL)
    assert a.shape == (2, 5, 64)
    assert torch.equal(a[:, :3], b[:, :3]) and not torch.equal(a[:, 3:], b[:, 3:])


def test_stage_references_compose_to_the_oracle():
    """The fp64 per-stage statement the codec kernel tests hold each stage to (oracle/codec_stages.py), composed stem -> stages ->
    head, equals codec_oracle's decode / encode on the same fp64 weights: the stage references are pinned to the oracle's
    formulation.  Specs cover biases and layer scales absent, a final norm, k = 5 and odd ratios."""
    from oracle import codec_stages as CS
    specs = (SMALL, CodecSpec(n_filters=8, ratios=(5, 3, 2), dec_depths=(1, 2, 1, 1), kernel=5, conv_bias=False, ffn_bias=False,
                              layer_scale=False, final_norm=True))
    g = torch.Generator().manual_seed(5)
    for spec in specs:
        wd = CS.f64(to_torch(synth_state_dict(codec_decoder_param_specs(spec), 2)))
        we = CS.f64(to_torch(synth_state_dict(codec_encoder_param_specs(spec), 2)))
        lat = torch.randn(3, 7, 64, generator=g, dtype=torch.float64)
        with torch.no_grad():
            ref, got = CO.decode(wd, lat, spec), CS.decode(wd, lat, spec)
        assert got.shape == ref.shape == (3, 1, spec.hop * 7)
        assert float((got - ref).norm() / ref.norm()) < 1e-12
        audio = torch.randn(3, 1, spec.hop * 6 + 2, generator=g, dtype=torch.float64) * 0.3
        with torch.no_grad():
            ref, got = CO.encode(we, audio, spec), CS.encode(we, audio, spec)
        assert got.shape == ref.shape == (3, 6, 64)
        assert float((got - ref).norm() / ref.norm()) < 1e-12
