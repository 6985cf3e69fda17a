"""CPU: what the recogniser / CTC tests rest on: the restatements of tests/helpers/asr_ref.py against torch's own ctc_loss,
the stated deviation (row alone vs torchaudio's batched form), the synthetic recipe, the checkpoint conversion and the Takes(ctc=)
validation."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from smalltts_amd import convert
from smalltts_amd.api import Repair, Takes, check_takes_ctc, phoneme_error_rate
from smalltts_amd.weights import all_param_specs, asr_param_specs, init_rule, load_weight_file, synth_state_dict
from tests.helpers import asr_ref as R

C = 198


@pytest.mark.parametrize("T,L,kind", [(1, 1, "distinct"), (4, 4, "distinct"), (7, 4, "equal"), (6, 4, "equal"), (395, 198, "equal"),
                                      (900, 198, "random")])
def test_ctc_restatement_equals_torch_ctc_loss_in_fp64(T, L, kind):
    g = torch.Generator().manual_seed(100 * T + L)
    logp = torch.randn(T, C, generator=g).log_softmax(-1).float()
    tgt = list(range(3, 3 + L)) if kind == "distinct" else [17] * L if kind == "equal" else torch.randint(1, C, (L,), generator=g).tolist()
    want = float(F.ctc_loss(logp.double()[:, None], torch.tensor([tgt]), torch.tensor([T]), torch.tensor([L]), blank=0,
                            reduction="none", zero_infinity=False))
    got = R.ctc_nll(logp.numpy(), T, tgt)
    if (T, L) == (6, 4):
        assert np.isposinf(want) and np.isposinf(got)
    else:
        assert np.isfinite(want) and abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)


def test_ctc_restatement_defined_edges():
    lp = torch.randn(5, C).log_softmax(-1).numpy()
    assert np.isposinf(R.ctc_nll(lp, 0, [3])) and np.isposinf(R.ctc_nll(lp, 5, []))
    lp2 = lp.copy()
    lp2[2, :] = -np.inf
    assert np.isposinf(R.ctc_nll(lp2, 5, [3, 4]))         # -inf, never NaN
    lp2 = lp.copy()
    lp2[2, 0] = np.nan
    assert np.isnan(R.ctc_nll(lp2, 5, [3, 4]))
    assert R.clamp_window(-3, 40, 9) == (0, 9) and R.clamp_window(4, 2, 9) == (4, 2)


def test_greedy_restatement_on_hand_made_rows():
    def rows(classes):
        lp = np.full((len(classes), 6), -5.0, np.float32)
        for t, c in enumerate(classes):
            lp[t, c] = -0.1
        return lp
    assert R.greedy(rows([4, 4, 0, 4, 5, 5, 5, 0, 0, 3]), 10) == [4, 4, 5, 3]     # repeats separated by a blank stay two tokens
    assert R.greedy(rows([4, 4, 0, 4, 5, 5, 5, 0, 0, 3]), 2) == [4]
    assert R.greedy(rows([0, 0, 0]), 3) == [] and R.greedy(rows([1, 2]), 0) == []  # all blank, no frames
    assert R.greedy(np.zeros((4, 6), np.float32), 4) == []                         # all ties: the lowest class = blank
    tie = rows([1])
    tie[0, 2] = tie[0, 5] = 3.0
    assert R.greedy(tie, 1) == [2]                                                 # a tie: the lower class


def test_row_alone_equals_the_batched_form_unragged_and_differs_ragged():
    """The stated deviation: torchaudio's conv module is not masked, so a short row inside a ragged batch reads its padding."""
    m = R.build(3)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 6, 64, generator=g)
    rows, bat = R.logprobs_rows(m, x, [6, 6]), R.logprobs_batched(m, x, [6, 6])
    assert float((rows - bat).abs().max()) < 1e-12
    rows, bat = R.logprobs_rows(m, x, [6, 3]), R.logprobs_batched(m, x, [6, 3])
    assert float((rows[0] - bat[0]).abs().max()) < 1e-12                           # the full row is the same either way
    diff = float((rows[1, :12] - bat[1, :12]).abs().max())
    assert diff > 1e-2, diff                                                        # about 1.0 in practice
    assert not rows[1, 12:].any()
    p = rows[0].exp()                                                               # not degenerate under the synthetic recipe
    assert 3.5 < float(-(p * rows[0]).sum(-1).mean()) < np.log(C) and float(p.max(-1).values.mean()) < 0.5


def test_synthetic_recipe_touches_only_asr_names_and_keeps_variances_positive():
    specs = asr_param_specs()
    assert all(n.startswith("asr.") for n, _ in specs) and not any(n.startswith("asr.") for n, _ in all_param_specs())
    assert len(specs) == 2 + 7 * 32 + 2
    sd = synth_state_dict(specs, 3)
    var = [k for k in sd if k.endswith("running_var")]
    assert len(var) == 7 and all((sd[k] >= 0.5).all() and (sd[k] <= 1.5).all() for k in var)
    for seed in (0, 1, 2):
        assert all((v > 0).all() for k, v in synth_state_dict(specs, seed).items() if k.endswith("running_var"))
    assert init_rule("asr.encoder.conformer_layers.0.conv_module.sequential.3.weight", (64,)) == (1.0, 0.2)
    assert init_rule("asr.encoder.conformer_layers.0.conv_module.sequential.3.running_mean", (64,)) == (0.0, 0.1)
    assert init_rule("asr.encoder.conformer_layers.0.self_attn.in_proj_bias", (192,)) == (0.0, 0.1)
    assert init_rule("asr.proj.weight", (198, 64)) == (0.0, np.sqrt(3.0 / 64))


def test_convert_asr_checkpoint_round_trip_and_refusals(tmp_path):
    sd = R.build(5, torch.float32).state_dict()                                    # the reference's key names, num_batches_tracked included
    assert any(k.endswith("num_batches_tracked") for k in sd)
    ck, out = tmp_path / "asr.pt", tmp_path / "asr.smtts"
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ck)           # wrapped and prefixed, as a training run leaves it
    assert convert.main(["--asr-checkpoint", str(ck), "--out", str(out)]) == 0
    tensors, _ = load_weight_file(str(out))
    want = synth_state_dict(asr_param_specs(), 5)
    assert sorted(tensors) == sorted(want) and all(np.array_equal(tensors[k], want[k]) for k in want)
    torch.save(sd, ck)                                                              # bare
    rep = convert.convert_checkpoint(None, str(out), asr_checkpoint=str(ck))
    assert rep.ok and rep["matched"] == len(want) and not rep["unexpected"]
    less = {k: v for k, v in sd.items() if k != "encoder.conformer_layers.4.self_attn.in_proj_bias"}
    torch.save(less, ck)
    with pytest.raises(ValueError, match=r"asr\.encoder\.conformer_layers\.4\.self_attn\.in_proj_bias"):
        convert.convert_checkpoint(None, str(out), asr_checkpoint=str(ck))
    wrong = dict(sd)
    wrong["proj.weight"] = torch.zeros(197, 64)
    torch.save(wrong, ck)
    with pytest.raises(ValueError, match=r"asr\.proj\.weight has shape \(197, 64\), expected \(198, 64\)"):
        convert.convert_checkpoint(None, str(out), asr_checkpoint=str(ck))
    extra = dict(sd)
    extra["encoder.pos_enc.weight"] = torch.zeros(3)
    torch.save(extra, ck)
    assert convert.convert_checkpoint(None, str(out), asr_checkpoint=str(ck))["unexpected"] == ["asr.encoder.pos_enc.weight"]


def test_takes_ctc_validation():
    assert Takes(3).ctc == 0.0 and Takes(3) == Takes(3, ctc=0.0) and Takes(3, ctc=1.5).ctc == 1.5 and Takes(3, ctc=1) != Takes(3)
    for bad in (-0.5, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="ctc"):
            Takes(3, ctc=bad)
    assert check_takes_ctc("call", None, None, None) is False and check_takes_ctc("call", Takes(3), Repair(1), None) is False
    with pytest.raises(ValueError, match="repair"):
        check_takes_ctc("call", Takes(3, ctc=1.0), Repair(1), None)

    class NoAsr:
        def has(self, part):
            return part != "asr"
    with pytest.raises(ValueError, match="recogniser"):
        check_takes_ctc("call", Takes(3, ctc=1.0), None, NoAsr())


def test_phoneme_error_rate():
    assert phoneme_error_rate([1, 2, 3], [1, 2, 3]) == 0.0
    assert phoneme_error_rate([1, 3], [1, 2, 3]) == pytest.approx(1 / 3)
    assert phoneme_error_rate([1, 2, 4, 3], [1, 2, 3]) == pytest.approx(1 / 3)
    assert phoneme_error_rate([], [1, 2]) == 1.0 and phoneme_error_rate([], []) == 0.0 and phoneme_error_rate([1], []) == float("inf")
