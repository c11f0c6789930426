"""CPU reference of the SwiGLU encoder (SwiGLUFFNFused, extern/dinov2/layers/swiglu_ffn.py:54-72), composed from the oracle's own
pieces -- prepare_tokens, layer_norm, vit_attention, fuse -- with the block's MLP replaced by  w3(silu(x1) * x2), [x1 | x2] = w12(x).
A helper module, not a test: dtype-generic (float64 autograd runs through it), nothing under oracle/ changes.

`round16`: emulation of the 16-bit training modes on the CPU -- the operands of every product of a block's linear layers (forward, d input
and d weight) and q | k | v are rounded to that type, where the kernels round them; `storage16` also rounds what train_storage='16bit' keeps
in 16 bits (attention output, branch outputs, x12 and the hidden activation h, a product of two rounded factors)."""
import torch
import torch.nn.functional as F

from mst import hip
from oracle import mst_oracle as O


hidden_of = hip.swiglu_hidden


def unpair(img, hidden, group):
    """Inverse of hip.pack_swiglu's row pairing: an image [2 Hp, ...] with pairing group `group` -> [2 hidden, ...] in the reference's
    chunk(2) order, the padding dropped."""
    Hp = img.shape[0] // 2
    assert img.shape[0] == 2 * Hp and Hp % group == 0 and hidden <= Hp
    t = img.reshape(Hp // group, 2, group, *img.shape[1:]).transpose(0, 1).reshape(2, Hp, *img.shape[1:])
    return t[:, :hidden].reshape(2 * hidden, *img.shape[1:]).contiguous()


def silu(x):
    return x * torch.sigmoid(x)


def swiglu_ffn(x, w12, b12, w3, b3):
    """SwiGLUFFNFused.forward: x12 = w12(x); x1, x2 = chunk(2, -1); w3(silu(x1) * x2)."""
    x1, x2 = F.linear(x, w12, b12).chunk(2, dim=-1)
    return F.linear(silu(x1) * x2, w3, b3)


class _Round(torch.autograd.Function):
    """Storage rounding: the value kept (and read by the next kernel) is the 16-bit one; its gradient passes unchanged."""
    @staticmethod
    def forward(ctx, x, dtype):
        return x.to(dtype).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


class _Lin16(torch.autograd.Function):
    """nn.Linear as the 16-bit training step computes it (mst/train.py, _lin_fwd / _Grads._lin_bwd_16): both operands of each of the
    three products rounded to the 16-bit type, exact accumulation, the bias and its gradient unrounded."""
    @staticmethod
    def forward(ctx, x, w, b, dtype):
        xr, wr = x.to(dtype).to(x.dtype), w.to(dtype).to(w.dtype)
        ctx.save_for_backward(xr, wr)
        ctx.dtype = dtype
        return F.linear(xr, wr, b)

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        dyr = dy.to(ctx.dtype).to(dy.dtype)
        dw = dyr.reshape(-1, dyr.shape[-1]).t() @ xr.reshape(-1, xr.shape[-1])
        return dyr @ wr, dw, dy.reshape(-1, dy.shape[-1]).sum(0), None


def block(x, sd, p, heads, round16=None, storage16=False):
    """block.py:89-114 with the SwiGLU FFN -> (x, attention probabilities).  A block whose keys are the GELU MLP's (mlp.fc1 / fc2; no
    16-bit emulation) is the oracle's own vit_block: one encoder loop serves every one-block model of tests/test_swiglu_gpu.py."""
    if (p + ".mlp.fc1.weight") in sd:
        assert round16 is None
        return O.vit_block(x, sd, p, heads)
    if round16 is None:
        lin, keep = F.linear, (lambda t: t)
    else:
        lin = lambda t, w, b: _Lin16.apply(t, w, b, round16)
        keep = (lambda t: _Round.apply(t, round16)) if storage16 else (lambda t: t)
    xn = O.layer_norm(x, sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-6)
    if round16 is None:
        a, probs = O.vit_attention(xn, sd, p, heads)
    else:                                                                # O.vit_attention (attention.py:56-69) with the roundings of the 16-bit step
        n, N, C = xn.shape
        d = C // heads
        qkv = lin(xn, sd[p + ".attn.qkv.weight"], sd[p + ".attn.qkv.bias"]).reshape(n, N, 3, heads, d).permute(2, 0, 3, 1, 4)
        q, k, v = (_Round.apply(t, round16) for t in (qkv[0] * (d ** -0.5), qkv[1], qkv[2]))   # 'flash' keeps q | k | v in 16 bits
        probs = (q @ k.transpose(-2, -1)).softmax(dim=-1)
        a = keep(lin(keep((probs @ v).transpose(1, 2).reshape(n, N, C)), sd[p + ".attn.proj.weight"], sd[p + ".attn.proj.bias"]))
    if (p + ".ls1.gamma") in sd:
        a = a * sd[p + ".ls1.gamma"]
    x = x + a
    x12 = keep(lin(O.layer_norm(x, sd[p + ".norm2.weight"], sd[p + ".norm2.bias"], 1e-6), sd[p + ".mlp.w12.weight"], sd[p + ".mlp.w12.bias"]))
    x1, x2 = x12.chunk(2, dim=-1)
    h = keep(lin(keep(silu(x1) * x2), sd[p + ".mlp.w3.weight"], sd[p + ".mlp.w3.bias"]))
    if (p + ".ls2.gamma") in sd:
        h = h * sd[p + ".ls2.gamma"]
    return x + h, probs


def encode(sd, slices, depth, heads, keep="none", round16=None, storage16=False):
    """DinoVisionTransformer.forward with SwiGLU blocks on [n, H, W] slices -> (normalised CLS [n, E], maps as O.vit_encode keeps them)."""
    x = O.prepare_tokens(sd, slices)
    maps = []
    for i in range(depth):
        x, probs = block(x, sd, O._block_prefix(sd, i), heads, round16, storage16)
        if keep == "cls":
            maps.append(probs[:, :, :1].clone())
        elif keep == "full":
            maps.append(probs)
    return O.layer_norm(x, sd["encoder.norm.weight"], sd["encoder.norm.bias"], 1e-6)[:, 0], maps


def forward(sd, source, depth, heads, *, src_key_padding_mask=None, keep="none", round16=None, storage16=False,
            slice_fusion_type="transformer"):
    """DinoV2ClassifierSlice.forward (dino.py:110-167) with the SwiGLU encoder: O.forward's dict."""
    B, C, D, H, W = source.shape
    emb, maps = encode(sd, source.permute(0, 2, 1, 3, 4).reshape(B * D * C, H, W), depth, heads, keep, round16, storage16)
    out = O.fuse(sd, emb, B, D * C, slice_fusion_type=slice_fusion_type, src_key_padding_mask=src_key_padding_mask)
    out["vit_maps"] = maps
    return out


def grads(sd, source, depth, heads, target, dtype=torch.float64, **kw):
    """Autograd through `forward` in `dtype`: (loss, logits, {parameter: gradient or None, "<source>": d source})."""
    p = {k: (v.to(dtype).requires_grad_() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    x = source.to(dtype).requires_grad_()
    logits = forward(p, x, depth, heads, **kw)["logits"]
    loss = F.cross_entropy(logits, target)
    loss.backward()
    g = {k: v.grad for k, v in p.items() if v.is_floating_point()}
    g["<source>"] = x.grad
    return float(loss.detach()), logits.detach(), g
