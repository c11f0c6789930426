#!/usr/bin/env python3
"""sha256 of everything one training step produces, for bit-equality checks between two trees or two libraries (MST_HIP_LIB).

    python tools/train_step_digest.py CONFIG [--deterministic]        one JSON line: {"config", "arrays", "sha256", "each": {name: sha256}}
    python tools/train_step_digest.py --list                          the configuration names

One configuration per process (a fresh process per configuration is the point: nothing cached carries over).  Models and inputs come
from mst.synth; nothing outside the repository is read.  Hashed: the logits, the loss, every parameter gradient, the source gradient
where the configuration asks for it, and every floating-point buffer after the step (BatchNorm running statistics).  --deterministic
sets torch.use_deterministic_algorithms(True): the fixed-order reductions, under which a step is bit-reproducible; without it the atomic
kernels run and digests differ from run to run.  The unit_* configurations call the ResNet step's convolution + BatchNorm unit directly;
the resnet*_infer_* and resnet*_frozen_source_grad ones hash the inference forward and the frozen eval-mode source gradient.
"""
import hashlib
import json
import sys
import warnings
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "new-vit_amd")]
warnings.simplefilter("ignore")
import torch
from mst import synth

DINO_SHAPE = (2, 1, 4, 224, 224)
RESNET_SHAPE = (2, 1, 3, 96, 96)


def _sha(t: torch.Tensor) -> str:
    t = t.detach().contiguous().cpu().reshape(-1)
    return hashlib.sha256(str((t.dtype, t.numel())).encode() + t.view(torch.uint8).numpy().tobytes()).hexdigest()


def _dino(sd_kw=None, **kw):
    from mst.models import DinoV2ClassifierSlice
    m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, **kw)
    m.load_state_dict(synth.synth_state_dict("s", 0, **(sd_kw or {})))
    return m.cuda().train()


def _registers():
    """The hub's dinov2_vits14_reg layout at its stored grid (tests/test_deterministic_gpu.py::_registers)."""
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_registers=True)
    m.encoder = _ViT(384, 12, 6, img_size=56, num_register_tokens=4, layerscale=1.0, chunked=False)
    m.load_state_dict(synth.synth_state_dict("s", 23, img_size=56, layerscale=True, chunked=False, num_register_tokens=4), strict=True)
    return m.cuda().train()


def _resnet34(model=34, **kw):
    from mst.models import ResNetSliceTrans
    m = ResNetSliceTrans(in_ch=1, out_ch=2, pretrained=False, model=model, **kw)
    m.load_state_dict(synth.synth_resnet_state_dict(0, model, 2), strict=True)
    return m.cuda().train()


def _resnet50_plain(**kw):
    from mst.models import ResNet
    m = ResNet(in_ch=3, out_ch=2, spatial_dims=2, pretrained=False, model=50, **kw)
    m.load_state_dict(synth.synth_resnet_state_dict(9, 50, 2, slice_trans=False, fc_out=2), strict=True)
    return m.cuda().train()


def step(model, src, mask=None, autocast=None, source_grad=False):
    """One forward (inside an autocast region if asked) + cross-entropy + backward (outside it) -> {name: tensor}."""
    src = src.cuda().requires_grad_(source_grad)
    kw = {} if mask is None else {"src_key_padding_mask": mask.cuda()}
    if autocast is None:
        logits = model(src, **kw)
    else:
        with torch.autocast("cuda", dtype=autocast):
            logits = model(src, **kw)
    loss = torch.nn.functional.cross_entropy(logits, torch.arange(src.shape[0], device="cuda") % 2)
    loss.backward()
    out = {"logits": logits, "loss": loss}
    out.update({"grad:" + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
    if source_grad:
        out["grad:source"] = src.grad
    out.update({"buffer:" + k: b for k, b in model.named_buffers() if b.is_floating_point()})
    return out


def _dino_case(shape=DINO_SHAPE, seed=3, mask=None, autocast=None, frozen=False, build=_dino, **kw):
    def run():
        m = build(**kw)
        if frozen:                                       # saliency: no parameter asks for a gradient, the source does
            m.requires_grad_(False)
            m.eval()
        return step(m, synth.synth_volume(shape, seed), mask, autocast, source_grad=frozen)
    return run


def _resnet_case(build=_resnet34, env=None, **kw):
    def run():
        import os
        os.environ.update(env or {})
        x = synth.synth_volume(RESNET_SHAPE, 4)
        return step(build(**kw), x[:, 0] if build is _resnet50_plain else x)        # the plain ResNet reads [N, 3, H, W]
    return run


def _resnet_infer_case(build=_resnet34, save_attn=False, **kw):
    """The inference forward (eval mode, no_grad) through the public API: the logits, with save_attn also get_attention_maps()."""
    def run():
        x = synth.synth_volume(RESNET_SHAPE, 4)
        m = build(**kw).eval()
        with torch.no_grad():
            out = {"logits": m((x[:, 0] if build is _resnet50_plain else x).cuda(), save_attn=save_attn)}
        if save_attn:
            out["attention_maps"] = m.get_attention_maps()
        return out
    return run


def _resnet_frozen_case(**kw):
    """A frozen ResNetSliceTrans in eval mode: the logits and the gradient of the source volume."""
    def run():
        m = _resnet34(**kw).eval().requires_grad_(False)
        return step(m, synth.synth_volume(RESNET_SHAPE, 4), source_grad=True)
    return run


def _unit_case(storage16):
    """The 147-tap stem (3 channels, 7 x 7, stride 2, 3 -> 64 on 2 x 32 x 32 x 3, no gray fold) through the unit alone, in fp16."""
    def run():
        from mst import train_resnet as T
        from mst.models.resnet import _Conv
        torch.manual_seed(5)                             # _Conv draws its weights from the global generator
        conv, bn = _Conv(3, 64, 7).cuda(), torch.nn.BatchNorm2d(64).cuda()
        g = torch.Generator().manual_seed(6)
        x = torch.randn(2, 32, 32, 3, generator=g).cuda()
        dy = torch.randn(2 * 16 * 16, 64, generator=g).cuda()
        y, rec = T._conv_bn_fwd(x, conv, bn, 7, 2, 3, False, None, True, torch.float16, storage16)
        G = T._Grads()
        dx = T._conv_bn_bwd(G, rec, dy, False, True)
        assert dx is None
        out = {"y": y, "z": rec["z"], "mean": rec["mean"], "rstd": rec["rstd"], "dy_masked": dy}
        out.update({"grad:" + k: G.by_param[id(p)] for k, p in (("conv.weight", conv.weight), ("bn.weight", bn.weight), ("bn.bias", bn.bias))})
        out.update({"buffer:" + k: b for k, b in bn.named_buffers() if b.is_floating_point()})
        return out
    return run


def _mask():
    m = torch.zeros(2, 4, dtype=torch.bool)
    m[1, 2:] = True
    return m


FLASH16 = dict(train_precision="fp16", train_attention="flash")
CONFIGS = {
    # DINOv2 synth ViT-S at 2 x 1 x 4 x 224 x 224
    "dino_fp32_stored": _dino_case(train_precision="fp32"),
    "dino_fp16_stored": _dino_case(train_precision="fp16"),
    "dino_bf16_flash": _dino_case(train_precision="bf16", train_attention="flash"),
    "dino_fp16_flash_16bit": _dino_case(train_storage="16bit", **FLASH16),
    "dino_autocast_fp16": _dino_case(autocast=torch.float16),
    "dino_rope_mask_slice_pos": _dino_case(mask=_mask(), rotary_positional_encoding="RoPE", use_slice_pos_emb=True,
                                           sd_kw=dict(rotary="RoPE", use_slice_pos_emb=True)),
    # (the 'linear' head is built for 32 slices: 1 x 1 x 32 x 224 x 224)
    "dino_fusion_linear": _dino_case(shape=(1, 1, 32, 224, 224), slice_fusion="linear", sd_kw=dict(slice_fusion="linear")),
    "dino_fusion_average": _dino_case(slice_fusion="average", sd_kw=dict(slice_fusion="average")),
    "dino_frozen_source_grad": _dino_case(frozen=True, **FLASH16),
    # other shapes: register tokens at their stored grid; 12,336 tokens (the transposed weight-gradient path above 12,288)
    "dino_registers": _dino_case(shape=(2, 1, 3, 56, 56), seed=123, build=_registers),
    "dino_12336_tokens_fp16_flash_fp32": _dino_case(shape=(1, 1, 48, 224, 224), **FLASH16),
    "dino_12336_tokens_fp16_flash_16bit": _dino_case(shape=(1, 1, 48, 224, 224), train_storage="16bit", **FLASH16),
    # ResNet at 2 x 1 x 3 x 96 x 96
    "resnet34_slice_fp32": _resnet_case(train_precision="fp32"),
    "resnet34_slice_fp16_fp32": _resnet_case(train_precision="fp16"),
    "resnet34_slice_fp16_16bit": _resnet_case(train_precision="fp16", train_storage="16bit"),
    "resnet34_slice_bf16_16bit": _resnet_case(train_precision="bf16", train_storage="16bit"),
    "resnet50_plain_fp16_fp32": _resnet_case(_resnet50_plain, train_precision="fp16"),
    "resnet50_plain_fp16_16bit": _resnet_case(_resnet50_plain, train_precision="fp16", train_storage="16bit"),
    "resnet34_slice_fp32_im2col": _resnet_case(env={"MST_CONV_IM2COL": "1"}, train_precision="fp32"),
    # ResNet inference forward and frozen eval-mode source gradient at the same shape (6 images: chunk_images=4 leaves a ragged chunk of 2)
    "resnet34_infer_fp32": _resnet_infer_case(),
    "resnet34_infer_bf16": _resnet_infer_case(compute_dtype="bf16"),
    "resnet50_plain_infer_fp16": _resnet_infer_case(_resnet50_plain, compute_dtype="fp16"),
    "resnet34_infer_save_attn": _resnet_infer_case(save_attn=True),
    "resnet34_infer_chunk4": _resnet_infer_case(chunk_images=4),
    "resnet34_frozen_source_grad": _resnet_frozen_case(),
    "resnet50_frozen_source_grad": _resnet_frozen_case(model=50),
    "unit_stem147_fp16_fp32": _unit_case(False),
    "unit_stem147_fp16_16bit": _unit_case(True),
}


def main():
    if "--list" in sys.argv:
        print("\n".join(CONFIGS))
        return
    name = sys.argv[1]
    if "--deterministic" in sys.argv:
        torch.use_deterministic_algorithms(True)
    out = CONFIGS[name]()
    torch.cuda.synchronize()
    each = {k: _sha(v) for k, v in out.items()}
    total = hashlib.sha256("".join(k + each[k] for k in sorted(each)).encode()).hexdigest()
    print(json.dumps({"config": name, "deterministic": torch.are_deterministic_algorithms_enabled(), "arrays": len(each), "sha256": total,
                      "each": each}), flush=True)


if __name__ == "__main__":
    main()
