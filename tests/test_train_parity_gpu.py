"""The fp32 HIP training step (mst/train.py, csrc/k_train.hip) against float64 autograd through the CPU oracle at the five cases of
tests/train_parity.py, with the atomic reductions and with the ordered ones (torch.use_deterministic_algorithms(True)):
loss, logits, every parameter gradient and the source gradient; under the flag a second step gives the same bits.  The bar (1e-4 of each
tensor's max |ref|) and why it can be trusted are in tests/train_parity.py and tests/test_train_parity_cpu.py."""
import pytest
import torch
import torch.nn.functional as F

import train_parity as P
from test_model_gpu import TOL, build

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[False, True], ids=["atomic", "deterministic"])
def det(request):
    prev, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(request.param)
    yield request.param
    torch.use_deterministic_algorithms(prev, warn_only=warn)


def _step(model, src, mask, target):
    model.zero_grad(set_to_none=True)
    source = src.cuda().requires_grad_()
    logits = model(source, src_key_padding_mask=mask)
    loss = F.cross_entropy(logits, target.cuda())
    loss.backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    grads[P.SOURCE] = source.grad
    return float(loss), logits.detach(), grads


@pytest.mark.parametrize("case", list(P.CASES))
def test_fp32_step_matches_float64_autograd(case, det):
    kw, src, mask, target = P.inputs(case)
    loss_ref, logits_ref, ref = P.oracle_grads(case, torch.float64)
    model = build(kw, P.STATE_SEED, "fp32").train()
    loss, logits, got = _step(model, src, mask, target)
    errs = P.scaled_errors(got, ref)
    worst = max(errs, key=errs.get)
    dlogits = float((logits.cpu().double() - logits_ref).abs().max())
    print(f"{case} deterministic={det}: worst scaled gradient error {errs[worst]:.3e} ({worst}), source {errs[P.SOURCE]:.3e}, "
          f"logits {dlogits:.3e}, loss {abs(loss - loss_ref):.3e}")
    assert abs(loss - loss_ref) < 1e-4
    assert dlogits < TOL["fp32"][0], dlogits
    for k, g in got.items():
        assert g is None or bool(torch.isfinite(g).all()), k
    P.check(got, ref)
    if det:
        got = {k: (None if g is None else g.clone()) for k, g in got.items()}
        _, logits2, again = _step(model, src, mask, target)
        assert torch.equal(logits2, logits)
        for k, g in got.items():
            assert (g is None and again[k] is None) or torch.equal(g, again[k]), k
