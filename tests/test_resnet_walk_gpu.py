"""The ResNet host walks (mst/models/resnet.py::backbone_chunk, mst/train_resnet.py::backbone_fwd): properties that hold because the
unit structure lives in one place.  Chunked inference gives the unchunked bits; the in-place residual sum never reaches the caller's
tensor; the eval-mode gradient forward is the fp32 inference forward whatever compute_dtype says; the training step's unit records
follow the block's chain.  Everything is bit equality (torch.equal): no tolerance to choose."""
import pytest
import torch

from mst import synth
from test_resnet_input_grad_gpu import _build
from test_resnet_storage_gpu import _deterministic

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("save_attn", [False, True], ids=["logits", "save_attn"])
@pytest.mark.parametrize("model", [18, 50])
def test_chunked_inference_gives_the_unchunked_bits(model, save_attn):
    """chunk_images = 4 over 6 images (a ragged last chunk of 2) against one chunk, fp32.  24 x 24 slices, the shape of
    test_frozen_eval_chunked_backbone_gives_the_same_bits: at most 1,024 rows per layer either way, so both forms stay on the same GEMM
    kernels.  (Not claimed for 16-bit compute_dtype or larger images: the chunk size may move a layer across _conv's routing rule.)"""
    seed, shape = 9, (1, 1, 6, 24, 24)
    src = synth.synth_volume(shape, seed + 100).cuda()
    out = {}
    for chunk in (128, 4):
        m, _ = _build("slice", model, seed, chunk_images=chunk)
        m = m.eval()
        with torch.no_grad():
            logits = m(src, save_attn=save_attn)
        out[chunk] = (logits,) + ((m.get_attention_maps(), m.get_slice_attention()) if save_attn else ())
    assert bool(torch.isfinite(out[128][0]).all()) and float(out[128][0].abs().max()) > 0
    for a, b in zip(out[128], out[4]):
        assert a.shape == b.shape and torch.equal(a, b)


def test_the_in_place_residual_never_reaches_the_caller():
    """ResNetSliceTrans.forward hands the walk a VIEW of a contiguous fp32 source on the device; the walk forms relu(identity + .) in place
    on dead activations only.  The source is unchanged after a forward and a second forward gives the same logits."""
    m, _ = _build("slice", 18, 7)
    m = m.eval()
    source = synth.synth_volume((2, 1, 3, 64, 64), 8).cuda().contiguous()
    assert source.dtype == torch.float32
    before = source.clone()
    with torch.no_grad():
        first = m(source)
        assert torch.equal(source, before)
        second = m(source)
    assert torch.equal(source, before) and torch.equal(first, second)


def test_the_gradient_forward_is_the_fp32_inference_forward_whatever_compute_dtype_says():
    """Model 50 at the slice50 case's shape, the same weights in a compute_dtype='bf16' model and an fp32 one, both frozen in eval mode.
    The bf16 model's logits with a source that requires grad are the fp32 model's no_grad logits, and its source gradient is the fp32
    model's (deterministic algorithms: the max-pool backward sums with atomics otherwise)."""
    seed, shape = 70, (1, 1, 2, 64, 64)
    src = synth.synth_volume(shape, seed + 105).cuda()
    m16, _ = _build("slice", 50, seed, compute_dtype="bf16")
    m32, _ = _build("slice", 50, seed)
    m16, m32 = m16.eval().requires_grad_(False), m32.eval().requires_grad_(False)
    with torch.no_grad():
        plain32, plain16 = m32(src), m16(src)
    assert not torch.equal(plain16, plain32), "the bf16 inference forward is not the fp32 one: the comparison below means something"
    grads = {}
    with _deterministic():
        for name, m in (("bf16", m16), ("fp32", m32)):
            source = src.clone().requires_grad_(True)
            logits = m(source)
            assert logits.grad_fn is not None
            logits[:, 1].sum().backward()
            grads[name] = (logits.detach(), source.grad)
    assert torch.equal(grads["bf16"][0], plain32) and torch.equal(grads["fp32"][0], plain32)
    assert float(grads["fp32"][1].abs().max()) > 0 and torch.equal(grads["bf16"][1], grads["fp32"][1])


@pytest.mark.parametrize("kind,model", [("slice", 18), ("plain", 50)])
def test_unit_records_follow_the_blocks_chain(kind, model):
    """One fp32 training forward: every sv["units"] entry is (the records of the unit's convolutions in forward order, then the downsample
    unit's record or None): 3 elements for a basic unit, 4 for a bottleneck."""
    from mst import train_resnet as T
    m, _ = _build(kind, model, 5)
    m = m.train()
    if kind == "slice":
        B, D = 2, 3
        x = synth.synth_volume((B, 1, D, 64, 64), 6).cuda().reshape(B * D, 64, 64, 1).contiguous()
    else:
        B = D = None
        x = torch.from_numpy(synth.hash_normal((6, 3, 64, 64), 6, 1)).float().cuda().permute(0, 2, 3, 1).contiguous()
    with torch.no_grad():
        _, sv = T.forward_train(m, x, kind == "slice", B, D, None)
    blocks = [blk for li in range(4) for blk in getattr(m.model, f"layer{li + 1}")]
    assert len(sv["units"]) == len(blocks)
    for blk, unit in zip(blocks, sv["units"]):
        convs = [blk.conv1, blk.conv2] + ([blk.conv3] if hasattr(blk, "conv3") else [])
        assert len(unit) == len(convs) + 1 == (4 if model >= 50 else 3)
        assert all(isinstance(r, dict) for r in unit[:-1]) and [r["conv"] for r in unit[:-1]] == convs
        if hasattr(blk, "downsample"):
            assert isinstance(unit[-1], dict) and unit[-1]["conv"] is blk.downsample[0]
        else:
            assert unit[-1] is None
