"""What the 1e-4 gradient bar of tests/train_parity.py means, shown on the CPU with the oracle alone: the reference's own fp32 rounding
stays 5x below it at every case, and an oracle with one modelled kernel defect (a mask bit, a RoPE position, one softmax key of 1370) moves
EVERY parameter's gradient above it -- so the bar neither fails a correct fp32 step nor passes one of these defects on any parameter."""
import pytest
import torch

import train_parity as P

NOISE = 2e-5    # fp32 oracle against fp64 oracle; measured worst over the five cases 1.1e-5 (grid_1x37).  Above this the bar has lost its margin


@pytest.mark.parametrize("case", list(P.CASES))
def test_fp32_noise_of_the_reference_is_far_below_the_bar(case):
    _, logits64, ref = P.oracle_grads(case, torch.float64)
    _, logits32, g32 = P.oracle_grads(case, torch.float32)
    assert all(v is None or v.dtype == torch.float64 for v in ref.values()) and logits64.dtype == torch.float64
    errs = P.check(g32, ref, bar=NOISE)
    dl = float((logits32.double() - logits64).abs().max())
    worst = max(errs, key=errs.get)
    print(f"{case}: fp32 noise worst {errs[worst]:.2e} ({worst}), source {errs[P.SOURCE]:.2e}, logits {dl:.2e}, "
          f"smallest gradient scale {min(float(ref[k].abs().max()) for k in errs):.2e}")
    assert dl <= NOISE, dl


@pytest.mark.parametrize("mutant", list(P.MUTANTS))
def test_mutant_moves_every_parameter_above_the_bar(mutant):
    case = P.MUTANTS[mutant][1]
    _, logits, ref = P.oracle_grads(case, torch.float64)
    _, mlogits, mut = P.oracle_grads(case, torch.float64, mutant)
    with pytest.raises(AssertionError, match="above"):
        P.check(mut, ref)
    errs = P.scaled_errors(mut, ref)
    low = min(errs, key=errs.get)
    print(f"{mutant} on {case}: min {errs[low]:.2e} ({low}), median {sorted(errs.values())[len(errs) // 2]:.2e}, "
          f"source {errs[P.SOURCE]:.2e}, logits moved by {float((mlogits - logits).abs().max()):.2e}")
    assert errs[low] > P.BAR, (low, errs[low])        # all of them, the source gradient included: not a share


def test_check_guards():
    _, _, ref = P.oracle_grads("slices70_rope", torch.float64)
    errs = P.check(ref, ref)
    assert max(errs.values()) == 0.0 and P.SOURCE in errs
    unused = [k for k, v in ref.items() if v is None]
    assert "encoder.mask_token" in unused and set(errs) == set(ref) - set(unused)
    name = "encoder.blocks.0.7.mlp.fc2.weight"
    with pytest.raises(AssertionError):                                   # one parameter missing
        P.check({k: v for k, v in ref.items() if k != name}, ref)
    with pytest.raises(AssertionError, match="no gradient"):              # ... or without a gradient
        P.check({**ref, name: None}, ref)
    with pytest.raises(AssertionError, match=name.replace(".", r"\.")):  # an all-zero gradient
        P.check({**ref, name: torch.zeros_like(ref[name])}, ref)
    with pytest.raises(AssertionError, match="reference has none"):      # a gradient for the unused mask_token
        P.check({**ref, "encoder.mask_token": torch.ones(1, 384)}, ref)
    P.check({**ref, "encoder.mask_token": torch.zeros(1, 384)}, ref)
    # one entry of one parameter off by 2e-4 of its scale is caught; by 0.5e-4 it is not
    for rel, ok in ((2e-4, False), (0.5e-4, True)):
        g = ref[name].clone()
        g.view(-1)[5] += rel * float(ref[name].abs().max())
        if ok:
            P.check({**ref, name: g}, ref)
        else:
            with pytest.raises(AssertionError, match="above"):
                P.check({**ref, name: g}, ref)
