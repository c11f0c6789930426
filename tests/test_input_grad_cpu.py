"""Host side of the source gradient (no GPU): the volume gradient goes back through the exact inverse of the training forward's input
layout -- [B, C, D, H, W] -> (b d c) slices, channel fastest (dino.py:125) -- and takes the source's dtype and device."""
import pytest
import torch

from mst import train


@pytest.mark.parametrize("shape", [(2, 1, 3, 28, 42), (1, 3, 2, 14, 28), (2, 2, 3, 14, 14)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_source_gradient_layout_is_the_adjoint_of_the_forward_reshape(shape, dtype):
    B, C, D0, H, W = shape
    x = torch.randn(shape)
    # what forward_train does to the source: channels become slices, channel fastest
    vol = (x.permute(0, 2, 1, 3, 4) if C != 1 else x).reshape(B * D0 * C, H, W).contiguous()
    g = train._source_grad(vol, {"src_shape": shape}, dtype, torch.device("cpu"))
    assert g.shape == x.shape and g.dtype == dtype and g.device.type == "cpu" and g.is_contiguous()
    assert torch.equal(g, x.to(dtype))
    # adjoint: <vol(x), v> = <x, vol^T(v)> for any v
    v = torch.randn(B * D0 * C, H, W, dtype=torch.float64)
    lhs = (vol.double() * v).sum()
    rhs = (x.double() * train._source_grad(v, {"src_shape": shape}, torch.float64, torch.device("cpu"))).sum()
    assert torch.allclose(lhs, rhs)
