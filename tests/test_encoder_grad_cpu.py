"""Gradients through the encoder API, the part that needs no GPU: where the bar of tests/test_encoder_grad_gpu.py comes from (the
reference alone), the three new C-ABI entries, and the ``encoder_grad`` switch on a CPU model."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import encoder_grad_ref as EG
from mst import hip

ROOT = Path(__file__).resolve().parent.parent


# ---- 1. the bar comes from the reference alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EG.CASES))
def test_fp32_noise_of_the_reference_is_a_fifth_of_the_bar_or_less(case):
    """The restatement in fp32 against itself in float64, the case's own loss: outputs and every gradient."""
    _, _, ref = EG.ref_grads(case)
    _, _, f32 = EG.ref_grads(case, torch.float32)
    errs = EG.scaled_errors(f32, ref)
    worst = max(errs, key=errs.get)
    print(f"{case}: fp32 noise {errs[worst]:.2e} ({worst}), x.grad {errs[EG.SOURCE]:.2e}")
    assert errs[worst] <= EG.BAR / 5, (worst, errs[worst])


@pytest.mark.parametrize("mutant", list(EG.MUTANTS))
def test_every_mutant_moves_its_parameter_five_bars_or_more(mutant):
    _, _, ref = EG.ref_grads("rgb_56x70")
    _, _, bad = EG.ref_grads("rgb_56x70", mutant=mutant)
    moved = EG.scaled_errors(bad, ref)
    aim = EG.MUTANTS[mutant]
    print(f"{mutant}: {aim} moved {moved[aim]:.2e}; {sum(m >= 5 * EG.BAR for m in moved.values())} of {len(moved)} by 5 bars or more")
    assert moved[aim] >= 5 * EG.BAR, (aim, moved[aim])
    with pytest.raises(AssertionError):
        EG.check(bad, ref)


def test_a_tap_behind_block_3_leaves_the_blocks_above_without_a_gradient():
    _, _, ref = EG.ref_grads("tap3_only")
    none = {k for k, g in ref.items() if g is None}
    assert "encoder.norm.weight" in none and "encoder.blocks.0.4.norm1.weight" in none and "encoder.blocks.0.11.mlp.fc2.bias" in none
    assert ref["encoder.blocks.0.3.mlp.fc2.bias"] is not None and ref["encoder.patch_embed.proj.weight"] is not None


# ---- 2. the C ABI --------------------------------------------------------------------------------------------------------------------
def _declared(header, name):
    m = re.search(rf"^int\s+{name}\s*\(([^;]*)\);", header, flags=re.M)
    assert m, f"{name} is not declared"
    return [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]


def test_rgb_patch_embedding_entries_are_declared_bound_and_exported():
    header = (ROOT / "include" / "mst_hip.h").read_text()
    assert _declared(header, "mst_patch_embed_rgb") == [
        "const float* img", "int n", "int H", "int W", "const float* wp", "const float* bias", "const float* prefix", "int n_prefix",
        "const float* pos_patch", "int E", "float* x", "mst_stream_t stream"]
    assert _declared(header, "mst_patch_embed_rgb_dgrad") == [
        "const float* dx", "int tokens_per_image", "int first_patch_token", "const float* wp", "int n", "int H", "int W", "int E",
        "float* dimg", "mst_stream_t stream"]
    assert _declared(header, "mst_patch_embed_rgb_wgrad") == [
        "const float* dx", "int tokens_per_image", "int first_patch_token", "const float* img", "int n", "int H", "int W", "int E",
        "int rows_per_split", "float* part", "mst_stream_t stream"]
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert hip.SIGNATURES["mst_patch_embed_rgb"] == (i, [vp, i, i, i, vp, vp, vp, i, vp, i, vp, vp])
    assert hip.SIGNATURES["mst_patch_embed_rgb_dgrad"] == (i, [vp, i, i, vp, i, i, i, i, vp, vp])
    assert hip.SIGNATURES["mst_patch_embed_rgb_wgrad"] == (i, [vp, i, i, vp, i, i, i, i, i, vp, vp])
    lib = hip.load()
    assert all(hasattr(lib, n) for n in ("mst_patch_embed_rgb", "mst_patch_embed_rgb_dgrad", "mst_patch_embed_rgb_wgrad"))
    assert lib.mst_version() == 300 == hip.ABI_VERSION                     # additions only
    # host-side argument checks run before anything touches a device
    assert lib.mst_patch_embed_rgb(None, 1, 28, 28, None, None, None, 1, None, 384, None, None) != 0
    assert "null pointer" in hip.last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.mst_patch_embed_rgb_dgrad(p, 4, 0, p, 1, 28, 30, 384, p, None) != 0 and "multiples of 14" in hip.last_error()
    assert lib.mst_patch_embed_rgb_dgrad(p, 3, 0, p, 1, 28, 28, 384, p, None) != 0 and "cannot hold" in hip.last_error()
    assert lib.mst_patch_embed_rgb_wgrad(p, 4, 0, p, 1, 28, 28, 384, 250, p, None) != 0 and "rows_per_split" in hip.last_error()
    assert lib.mst_patch_embed_rgb_wgrad(p, 4, 0, p, 1, 28, 28, 100, 256, p, None) != 0 and "multiple of 64" in hip.last_error()
    # the split rule the training step and the wgrad_splits case rely on
    assert [hip.rgb_wgrad_split_rows(r) for r in (1, 280, 4096, 4097, 87616)] == [256, 256, 256, 272, 5488]


# ---- 3. the switch ---------------------------------------------------------------------------------------------------------------------
def test_encoder_grad_is_a_constructor_keyword_and_an_attribute_and_no_state():
    from mst.models import DinoV2ClassifierSlice
    off = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False)
    on = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, encoder_grad=True)
    assert off.encoder_grad is False and on.encoder_grad is True
    assert list(on.state_dict()) == list(off.state_dict()) and not any("encoder_grad" in k for k in on.state_dict())
    on.encoder_grad = False
    assert on.encoder_grad is False


def test_a_cpu_model_with_the_switch_on_refuses_in_today_s_order():
    from mst.models import DinoV2ClassifierSlice
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, encoder_grad=True)
    enc = model.encoder
    x = torch.zeros(1, 3, 28, 28, requires_grad=True)
    assert torch.is_grad_enabled() and any(p.requires_grad for p in enc.parameters())
    with pytest.raises(NotImplementedError, match="mask"):
        enc.forward_features(x, masks=torch.zeros(1, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="list"):
        enc.forward_features([x])
    with pytest.raises(NotImplementedError, match="mask"):
        enc(x, masks=torch.zeros(1, 4, dtype=torch.bool))
    for call in (lambda: enc(x), lambda: enc.forward_features(x), lambda: enc.get_intermediate_layers(x, n=[3], norm=False)):
        with pytest.raises(Exception, match="(?i)no CPU fallback"):
            call()
