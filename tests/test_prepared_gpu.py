"""A model whose parameter or buffer was edited in place computes, on its next forward, what a freshly constructed model loaded with
the edited ``state_dict`` computes -- bit for bit: every device-side weight image (packed encoder blocks, BatchNorm-folded
convolutions, the bound slice transformer) follows the edit (mst/models/prepared.py).  One edit at a time, under ``no_grad``."""
import warnings

import pytest
import torch

from mst import synth

pytestmark = pytest.mark.gpu


def _dino(sd):
    from mst.models import DinoV2ClassifierSlice
    m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="bf16")
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _resnet(sd):
    from mst.models import ResNet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ResNet(in_ch=3, out_ch=2, spatial_dims=2, model=18, pretrained=False, compute_dtype="fp32")
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _resnet_slice_trans(sd):
    from mst.models import ResNetSliceTrans
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ResNetSliceTrans(in_ch=1, out_ch=2, model=18, pretrained=False, compute_dtype="fp32")
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


FUSION_EDITS = {"final norm": lambda m: m.slice_fusion.norm.weight.mul_(1.5), "cls_token": lambda m: m.cls_token[..., ::2].add_(1.0)}
BACKBONE_EDITS = {"conv weight": lambda m: m.model.layer4[1].conv2.weight.mul_(1.5),
                  "running_var": lambda m: m.model.layer4[1].bn2.running_var.mul_(2.0)}
CASES = {
    "dino": (_dino, lambda: synth.synth_state_dict("s", 0), lambda: synth.synth_volume((1, 1, 4, 112, 112), 123),
             {"encoder weight": lambda m: m.encoder.block_list()[-1].mlp.fc2.weight.mul_(1.5), **FUSION_EDITS}),
    "resnet": (_resnet, lambda: synth.synth_resnet_state_dict(7, 18, 2, slice_trans=False, fc_out=2),
               lambda: torch.from_numpy(synth.hash_normal((2, 3, 64, 64), 8, 1)), BACKBONE_EDITS),
    "resnet_slice_trans": (_resnet_slice_trans, lambda: synth.synth_resnet_state_dict(7, 18, 2),
                           lambda: synth.synth_volume((1, 1, 4, 64, 64), 9), {**BACKBONE_EDITS, **FUSION_EDITS}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_forward_after_an_in_place_edit_equals_a_fresh_model(case):
    make, state_dict, source, edits = CASES[case]
    x = source()
    with torch.no_grad():
        model = make(state_dict())
        before = model(x)
        for name, edit in edits.items():
            edit(model)
            got = model(x)
            want = make({k: v.detach().clone() for k, v in model.state_dict().items()})(x)
            print(f"{case}, {name}: max|logits - fresh| {float((got - want).abs().max()):.3e}, "
                  f"max|logits - before| {float((got - before).abs().max()):.3e}")
            assert torch.equal(got, want), name
            assert not torch.equal(got, before), name
            before = got
