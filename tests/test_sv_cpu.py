"""CPU: what the verifier tests rest on: the inventory and the synthetic recipe, the restatement of tests/helpers/sv_ref.py
(a row alone against the ragged batch, the stated deviation from speechbrain's batched form, the n = 5 refusal), the checkpoint
conversion, the Takes(sv=) validation and the header's new entries."""
import numpy as np
import pytest
import torch

from smalltts_amd import _lib, convert
from smalltts_amd.api import Repair, Takes, Voice, check_takes_sv
from smalltts_amd.weights import all_param_specs, init_rule, load_weight_file, sv_param_specs, synth_state_dict
from tests.helpers import sv_ref as R


def test_inventory_names_shapes_and_parameter_count():
    specs = sv_param_specs()
    names = [n for n, _ in specs]
    assert len(set(names)) == len(names) and all(n.startswith("sv.ecapa.") for n in names)
    assert not any(n.startswith("sv.") for n, _ in all_param_specs())              # an optional part, like the recogniser
    stats = sum(int(np.prod(s)) for n, s in specs if n.endswith(("running_mean", "running_var")))
    total = sum(int(np.prod(s)) for _, s in specs)
    assert total - stats == 12_983_808 and stats == 2 * 14_592                     # parameters, and the BatchNorm statistics apart
    d = dict(specs)
    assert d["sv.ecapa.blocks.0.conv.conv.weight"] == (768, 64, 3) and d["sv.ecapa.blocks.3.res2net_block.blocks.10.conv.conv.weight"] == (64, 64, 3)
    assert d["sv.ecapa.blocks.2.se_block.conv1.conv.weight"] == (192, 768, 1) and d["sv.ecapa.blocks.2.se_block.conv2.conv.bias"] == (768,)
    assert d["sv.ecapa.mfa.conv.conv.weight"] == (2304, 2304, 1) and d["sv.ecapa.asp.tdnn.conv.conv.weight"] == (192, 6912, 1)
    assert d["sv.ecapa.asp.conv.conv.weight"] == (2304, 192, 1) and d["sv.ecapa.asp_bn.norm.running_var"] == (4608,)
    assert d["sv.ecapa.fc.conv.weight"] == (192, 4608, 1) and "sv.ecapa.blocks.1.res2net_block.blocks.11.conv.conv.weight" not in d
    assert not any("num_batches_tracked" in n for n in names)
    assert sorted(k for k in R.SVRef().state_dict() if not k.endswith("num_batches_tracked")) == sorted(n[len("sv."):] for n in names)


def test_synthetic_recipe_keeps_variances_positive_and_activations_alive():
    specs = sv_param_specs()
    for seed in (0, 1, 5):
        sd = synth_state_dict(specs, seed)
        assert all((v >= 0.5).all() and (v <= 1.5).all() for k, v in sd.items() if k.endswith("running_var"))
        assert all((v >= 0.8).all() for k, v in sd.items() if k.endswith("norm.weight"))
    assert init_rule("sv.ecapa.mfa.conv.conv.weight", (2304, 2304, 1)) == (0.0, np.sqrt(6.0 / 2304))       # He-style: a ReLU follows
    assert init_rule("sv.ecapa.blocks.1.res2net_block.blocks.0.conv.conv.weight", (64, 64, 3)) == (0.0, np.sqrt(6.0 / 192))
    assert init_rule("sv.ecapa.fc.conv.weight", (192, 4608, 1)) == (0.0, np.sqrt(3.0 / 4608))              # no ReLU behind it
    assert init_rule("sv.ecapa.asp_bn.norm.running_mean", (4608,)) == (0.0, 0.1)
    m = R.build(5)
    x = torch.randn(2, 30, 64, generator=torch.Generator().manual_seed(2))
    e = R.embed_rows(m, x, [30, 12])
    assert torch.isfinite(e).all() and 1.0 < float(e.abs().max()) < 1e4 and float(e.std()) > 0.1            # neither dead nor blown up
    assert 0.0 < R.cosine(e[:1].numpy(), e[1:].numpy())[0] < 1.0


def test_a_row_alone_equals_the_row_inside_a_ragged_batch_exactly_and_the_batched_form_differs():
    """The stated rule (every row as if alone) and why it exists: speechbrain's batched form masks the squeeze-excite mean and the
    pooling but not the convolutions, which reflect about the batch's end and read a short row's padding."""
    m = R.build(5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 12, 64, generator=g)
    lens = [12, 7, 6]
    rows = R.embed_rows(m, x, lens)
    for b, n in enumerate(lens):
        alone = R.embed_rows(m, x[b:b + 1, :n].clone(), [n])
        assert torch.equal(alone[0], rows[b])                                       # exactly, in fp64
    garbage = x.clone()
    garbage[1, 7:] = float("nan")
    garbage[2, 6:] = 1e30
    assert torch.equal(R.embed_rows(m, garbage, lens), rows)                        # nothing behind the length is read
    bat = R.embed_batched(m, x, lens)
    assert float((bat[0] - rows[0]).abs().max()) < 1e-9 * float(rows[0].abs().max())   # the full row: the same either way
    assert float((bat[1] - rows[1]).abs().max()) > 1e-3 * float(rows[1].abs().max())   # the short rows: not
    assert float((R.embed_batched(m, x, [12, 12, 12]) - R.embed_rows(m, x, [12, 12, 12])).abs().max()) < 1e-9 * float(rows.abs().max())


def test_five_frames_are_refused_and_have_no_embedding():
    m = R.build(5)
    x = torch.randn(1, 6, 64, generator=torch.Generator().manual_seed(3))
    with pytest.raises(RuntimeError, match="[Pp]adding"):
        m(x[:, :5].double())
    assert torch.isfinite(m(x.double())).all()
    assert not R.embed_rows(m, x, [5]).any() and R.embed_rows(m, x, [6]).any()
    assert R.cosine(np.zeros((1, 192)), np.ones((1, 192)))[0] == 0.0                # F.cosine_similarity's rule: a zero row gives 0


def test_convert_sv_checkpoint_round_trip_and_refusals(tmp_path):
    sd = R.build(5, torch.float32).state_dict()                                    # the reference's key names, num_batches_tracked included
    assert any(k.endswith("num_batches_tracked") for k in sd)
    ck, out = tmp_path / "sv.pt", tmp_path / "sv.smtts"
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ck)           # wrapped and prefixed, as train/dmd2/sv.py leaves it
    assert convert.main(["--sv-checkpoint", str(ck), "--out", str(out)]) == 0
    tensors, _ = load_weight_file(str(out))
    want = synth_state_dict(sv_param_specs(), 5)
    assert sorted(tensors) == sorted(want) and all(np.array_equal(tensors[k], want[k]) for k in want)
    torch.save(sd, ck)                                                              # bare
    rep = convert.convert_checkpoint(None, str(out), sv_checkpoint=str(ck))
    assert rep.ok and rep["matched"] == len(want) and not rep["unexpected"]
    less = {k: v for k, v in sd.items() if k != "ecapa.blocks.2.se_block.conv2.conv.bias"}
    torch.save(less, ck)
    with pytest.raises(ValueError, match=r"sv\.ecapa\.blocks\.2\.se_block\.conv2\.conv\.bias"):
        convert.convert_checkpoint(None, str(out), sv_checkpoint=str(ck))
    wrong = dict(sd)
    wrong["ecapa.fc.conv.weight"] = torch.zeros(192, 4607, 1)
    torch.save(wrong, ck)
    with pytest.raises(ValueError, match=r"sv\.ecapa\.fc\.conv\.weight has shape \(192, 4607, 1\), expected \(192, 4608, 1\)"):
        convert.convert_checkpoint(None, str(out), sv_checkpoint=str(ck))
    extra = dict(sd)
    extra["ecapa.blocks.0.dropout.p"] = torch.zeros(3)
    torch.save(extra, ck)
    assert convert.convert_checkpoint(None, str(out), sv_checkpoint=str(ck))["unexpected"] == ["sv.ecapa.blocks.0.dropout.p"]
    with pytest.raises(SystemExit):
        convert.main(["--onnx", "a.onnx", "--sv-checkpoint", str(ck), "--out", str(out)])


def test_takes_sv_validation_repr_equality_and_hash():
    assert Takes(3).sv == 0.0 and Takes(3) == Takes(3, sv=0.0) and Takes(3, sv=1.5).sv == 1.5 and Takes(3, sv=1) != Takes(3)
    assert Takes(3, ctc=1.0, sv=2.0) != Takes(3, ctc=2.0, sv=1.0) and hash(Takes(3, sv=0.5)) == hash(Takes(3, sv=0.5))
    assert len({Takes(3), Takes(3, sv=0.0), Takes(3, sv=0.5), Takes(3, ctc=0.5)}) == 3
    assert repr(Takes(2, sv=0.25)).endswith("ctc=0.0, sv=0.25)")
    for bad in (-0.5, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="sv"):
            Takes(3, sv=bad)
    with pytest.raises(AttributeError):
        Takes(3).sv = 1.0

    class Eng:
        def __init__(self, sv):
            self.sv = sv

        def has(self, part):
            return part != "sv" or self.sv
    yes, no = Eng(True), Eng(False)
    assert check_takes_sv("call", None, None, no) is False and check_takes_sv("call", Takes(3), Repair(1), no) is False
    assert check_takes_sv("call", Takes(3, sv=1.0), None, yes, [6, 225], None, [6, 225]) is True
    with pytest.raises(ValueError, match="repair"):
        check_takes_sv("call", Takes(3, sv=1.0), Repair(1), yes)
    with pytest.raises(ValueError, match="verifier"):
        check_takes_sv("call", Takes(3, sv=1.0), None, no)
    for ns in ([9, 5], [226], [0]):
        with pytest.raises(ValueError, match="frames in every row"):
            check_takes_sv("call", Takes(3, sv=1.0), None, yes, ns)
    with pytest.raises(ValueError, match="reference frames"):
        check_takes_sv("call", Takes(3, sv=1.0), None, yes, [9], None, [5])
    k = torch.zeros(12, 1, 8, 4, 120)
    v = Voice(yes, k, k)                                                            # the three-argument form keeps working
    assert v.speaker is None and v.R == 4
    with pytest.raises(ValueError, match="speaker embedding"):
        check_takes_sv("call", Takes(3, sv=1.0), None, yes, [9], [v])
    spk = torch.zeros(192)
    assert check_takes_sv("call", Takes(3, sv=1.0), None, yes, [9], [Voice(yes, k, k, spk)]) is True
    with pytest.raises(AttributeError):
        v.speaker = spk


def test_the_header_declares_the_new_entries_and_the_abi_number_stays():
    syms = _lib.header_symbols()
    for name in ("smtts_sv_workspace_bytes", "smtts_sv_embed", "smtts_sv_cosine"):
        assert name in _lib.SIGNATURES and name in syms
    assert len(_lib.SIGNATURES["smtts_sv_embed"][1]) == 9 and len(_lib.SIGNATURES["smtts_sv_cosine"][1]) == 8
    assert _lib.ABI_VERSION == 11


def test_a_wrong_sv_shape_is_refused_by_name_before_it_reaches_the_packers():
    """The host half of the shape checks (finalize checks every sv. shape by name on the device side, tests/test_sv_bounds_gpu.py
    loads the part): a weight file of another model size is a clean error naming the tensor."""
    from smalltts_amd.api import _validated
    from smalltts_amd.weights import DEFAULT_CODEC
    good = {n: np.zeros(s, np.float32) for n, s in sv_param_specs()[:6]}
    assert _validated(good, "sv.smtts", DEFAULT_CODEC) is not None
    for name, shape in (("sv.ecapa.fc.conv.weight", (192, 4607, 1)), ("sv.ecapa.blocks.1.res2net_block.blocks.3.conv.conv.weight", (64, 64, 5)),
                        ("sv.ecapa.asp_bn.norm.running_var", (2304,))):
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            _validated({**good, name: np.zeros(shape, np.float32)}, "sv.smtts", DEFAULT_CODEC)
