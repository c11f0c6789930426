"""Training step of ResNet / ResNetSliceTrans on the HIP path (BASELINE configs[3]).

The reference trains these through torch.autograd over torchvision's modules (mst/models/base_model.py:148-181 `_step`,
mst/models/resnet.py:172-193).  Here, as for DinoV2ClassifierSlice (mst/train.py), the logits carry ONE autograd node whose
forward runs the model op by op through the C ABI and whose backward produces every parameter gradient with HIP kernels:

  convolution      z = im2col(x) . Wg^T             (mst_conv_gemm: implicit GEMM, exact fp32 MFMA; the stem: mst_im2col_nhwc + mst_gemm;
                                                     Wg = weight in (ky, kx, c) order)
     backward      dWg = dz^T . im2col(x) as an implicit GEMM too (mst_conv_wgrad: pixel-split partial products reduced by mst_colsum),
                   dx = the stride-1 convolution of the stride-dilated dz with the flipped, transposed weight (mst_conv_dgrad); the
                   stem's dW and MST_CONV_IM2COL=1 keep the explicit forms (mst_im2col_nhwc + mst_gemm_ex, mst_col2im_nhwc); the stem's
                   dx -- only when the source asks for a gradient -- is mst_conv_dgrad_stem (per-tile dz . Wg in LDS, gathered: no atomics)
     16-bit        a 16-bit train_precision: the three products on 16-bit MFMA operands with fp32 accumulation (mst_conv_gemm16,
                   mst_conv_dgrad, mst_conv_wgrad16)
  BatchNorm2d      batch statistics + running-stat update, residual add and ReLU in the same pass: hip.batchnorm_train, which takes the
                   entry point by z's dtype (csrc/k_bn.hip: one kernel family, one host sequence for every mode)
     backward      mst_batchnorm_bwd (ReLU mask first: mst_act_bwd on the saved output)
     16-bit stored train_storage='16bit': mst_batchnorm_train16, ONE mst_batchnorm_bwd16 per unit (it takes the mask from the saved y)
  max / avg pool   mst_maxpool_bwd_nhwc / mst_avgpool_bwd_nhwc (csrc/k_bn.hip as well; by the input's dtype)
  slice fusion     mst.train.fusion_fwd / fusion_bwd with 16 heads over 512-wide tokens

BatchNorm in train mode normalises over ALL (B D) images of the step, so the step is not chunked: activations of the whole batch stay
resident (fp32 NHWC; about 60 MB per 224^2 image for resnet34 -- sized for 288 GB of HBM; the mixed mode keeps a 16-bit image of every
convolution input beside it).  Checked against torch.autograd of oracle/resnet_oracle.py on every parameter (tests/test_resnet_gpu.py).

Gradient with respect to the input volume: the node returns d x_nhwc when its source requires grad (`backbone_bwd(need_source=True)`),
and torch carries it through the model's own float() / permute / reshape to the source's shape, dtype and device.  The backward is pruned
to what is asked for (`_Grads(needed=...)` from needs_input_grad): a frozen model's source-only backward forms no weight gradient.  A frozen
model in eval mode has its own node on the BatchNorm-folded weights (`_ResNetEvalFunction`, fp32); its forward IS the inference walk
(mst/models/resnet.py::backbone_chunk, with a keep list), chunked like it.
Checked against float64 torch.autograd through the oracle (tests/test_resnet_input_grad_gpu.py).

What a residual unit is lives in one place, `_Unit.chain()` / `_Unit.shortcut()` (mst/models/resnet.py): `backbone_fwd` / `backbone_bwd`
walk that chain over `_conv_bn_fwd` records, `_eval_backbone_bwd` walks it over the `Folded` records, which carry k, stride and pad.

The mode (train_precision, train_storage and the autocast rule) is described, validated and resolved in mst/train_mode.py;
`forward_train` resolves it once and the saved state and every unit's record carry it to the backward.

Determinism: under ``torch.use_deterministic_algorithms(True)`` (read at every call) the BatchNorm statistics and their gradients
(mst_batchnorm_train_ordered / mst_batchnorm_bwd_ordered), the weight-gradient partial sums (mst_colsum_ordered), col2im and the max-pool
backward (gather forms: every input sums its own contributions in a fixed order) run without floating-point atomics, so a step -- logits,
loss, gradients, running statistics -- is bit-reproducible.  Flag off: the atomic kernels, as before.
"""
from __future__ import annotations

import os
from typing import Optional, Set

import torch
import torch.nn as nn

from . import hip, train_mode
from .models.resnet import SLICE_HEADS, _conv, backbone_chunk, conv_out
from .train import _Grads, fp32_device_params, fusion_bwd, fusion_fwd, route_grads


def _gemm_weight(conv, sum_in: bool) -> torch.Tensor:
    """[Cout, Cin, kh, kw] -> [Cout, Kpad] in (ky, kx, c) order (identical input channels summed when the gray volume was repeated)."""
    w = conv.weight.detach()
    if sum_in:
        w = w.sum(dim=1, keepdim=True)
    w = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    K = w.shape[1]
    kpad = (K + 15) // 16 * 16
    if kpad != K:
        w = torch.cat([w, w.new_zeros(w.shape[0], kpad - K)], dim=1)
    return w.contiguous()


def _conv_bn_fwd(x: torch.Tensor, conv, bn, k: int, stride: int, pad: int, sum_in: bool, residual: Optional[torch.Tensor],
                 relu: bool, mp: Optional[torch.dtype] = None, storage16: bool = False):
    """x [n,H,W,C] -> y [n,Ho,Wo,Cout] plus the record the backward needs.  mp (a 16-bit train_precision): the convolution and its two
    gradients on 16-bit MFMA operands (fp32 accumulation) -- the reference's Trainer(precision='16-mixed') for F.conv2d.  A unit that
    cannot take them runs in fp32 and records mp = None.  storage16 (train_storage='16bit', needs mp): x ALREADY in mp (the producer's y;
    the stem: the fp32 source images), residual [rows, Cout] in mp, z and y in mp; the record then keeps nothing fp32 but the [C]
    statistics and no copy of the input, and a unit that cannot take the 16-bit products is a ValueError."""
    if storage16 and mp is None:
        train_mode.check(False, "stored", "16bit", needs_flash=False)        # raises: 16-bit storage without a 16-bit type
    n, H, W, Cin = x.shape
    wg = _gemm_weight(conv, sum_in)
    Ho, Wo = conv_out(H, k, stride, pad), conv_out(W, k, stride, pad)
    Cout, K = wg.shape[0], k * k * Cin
    zdt = mp if storage16 else torch.float32
    x16 = col16 = None
    if mp is not None and Cin % 64 == 0 and Cout % 64 == 0 and (x.dtype == mp or not storage16):
        # the operand image: x itself, or a 16-bit copy kept for the weight gradient (a third of the step's conversions otherwise)
        x16 = x if storage16 else hip.cvt16(x.view(-1, Cin), mp).view(x.shape)
        z = hip.conv_gemm16(x16, hip.cvt16(wg, mp), None, k, k, stride, pad, epilogue=hip.EPI_BIAS, out_dtype=zdt)
    elif mp is not None and Cout % 64 == 0 and x.dtype == torch.float32 and (storage16 or K <= 64):
        # the stem (49 taps after the gray fold; with 16-bit storage also the 147 of three channels, which fp32 storage leaves to the fp32
        # implicit GEMM): its im2col rows, rounded on the way out and padded to a multiple of 64 columns, are the "pixels" of a 1 x 1
        # convolution -- for the forward and for the weight gradient (no fp32 im2col matrix, no strided fp32 GEMM)
        kp = (K + 63) // 64 * 64
        w64 = torch.zeros((Cout, kp), dtype=torch.float32, device=x.device)
        w64[:, :K] = wg[:, :K]
        col16 = hip.im2col_nhwc(x, k, k, stride, pad, kp, out_dtype=mp).view(n * Ho * Wo, 1, 1, kp)
        z = hip.conv_gemm16(col16, hip.cvt16(w64, mp), None, 1, 1, 1, 0, epilogue=hip.EPI_BIAS, out_dtype=zdt)
    elif storage16:
        raise ValueError(f"train_storage='16bit': a {k} x {k} convolution {Cin} -> {Cout} on a {x.dtype} input cannot take the 16-bit products "
                         "(behind the stem Cin and Cout must be multiples of 64 and the input already in the 16-bit type)")
    else:
        mp = None
        z = _conv(x, wg, None, k, stride, pad, wg.shape[1], hip.EPI_BIAS)    # implicit GEMM behind the stem
    y, mean, rstd = hip.batchnorm_train(z, bn, residual, relu)             # by z's dtype: fp32, or the 16-bit storage form
    bn.num_batches_tracked += 1
    rec = {"x": x, "z": z, "y": y if relu else None, "mean": mean, "rstd": rstd, "wg": None if storage16 else wg, "k": k, "stride": stride,
           "pad": pad, "sum_in": sum_in, "relu": relu, "conv": conv, "bn": bn, "mp": mp, "x16": x16, "col16": col16, "storage16": storage16}
    return y.view(n, Ho, Wo, Cout), rec


def _split(n: int, hw: int):
    """Split the rows of one layer's im2col matrix for dW: (images, parts per image) with parts | hw, about 256 partial products."""
    s2 = 1
    while s2 < 16 and hw % (s2 * 2) == 0 and n * s2 < 256:
        s2 *= 2
    return n, s2


def _conv_bn_bwd(G: _Grads, rec, dy: torch.Tensor, need_dx: bool, mask_dy: bool = True) -> Optional[torch.Tensor]:
    """dy [rows, Cout] = gradient of the unit's output.  Returns dx [n,H,W,C] or None.  The caller routes the masked dy to the residual
    branch itself: fp32 storage always writes the ReLU mask into dy; 16-bit storage does so only with mask_dy (False: nobody reads the
    masked dy) and leaves the dy of a unit without ReLU alone."""
    x, z, wg, mp, st16 = rec["x"], rec["z"], rec["wg"], rec["mp"], rec["storage16"]
    conv, bn = rec["conv"], rec["bn"]
    k, stride, pad = rec["k"], rec["stride"], rec["pad"]
    n, H, W, Cin = x.shape
    rows, Cout = z.shape
    dev = z.device
    if st16:                                                             # ONE pass: ReLU mask from the saved y, both sums, dz rounded to mp
        dz = None
        dz16, dg, db = hip.batchnorm_bwd16(z, rec["y"], rec["mean"], rec["rstd"], bn.weight.detach(), dy, mask_dy and rec["relu"])
    else:
        if rec["relu"]:
            hip.act_bwd(rec["y"], dy, 1)
        dz, dg, db = hip.batchnorm_bwd(z, rec["mean"], rec["rstd"], bn.weight.detach(), dy)
        dz16 = hip.cvt16(dz, mp) if mp is not None else None            # shared by the two gradients
    G.put(bn.weight, dg)
    G.put(bn.bias, db)
    implicit = st16 or os.environ.get("MST_CONV_IM2COL", "0") != "1"    # the explicit im2col / col2im forms are fp32 storage's
    col = None
    dwg = None
    if not G.need(conv.weight):                                          # pruned (a frozen model's source-only backward): the d x chain alone
        pass
    elif rec["col16"] is not None:                                       # the stem's 16-bit product: d weight over its 16-bit im2col "pixels"
        dwg = hip.conv_wgrad(dz16, rec["col16"], 1, 1, 0)
        if not st16:                                                     # fp32 storage hands on a [Cout, kpad] matrix like its other forms
            kpad, dwg64 = wg.shape[1], dwg
            dwg = torch.zeros((Cout, kpad), dtype=torch.float32, device=dev)
            dwg[:, :min(kpad, 64)] = dwg64[:, :min(kpad, 64)]
    elif implicit and rec["x16"] is not None:
        dwg = hip.conv_wgrad(dz16, rec["x16"], k, stride, pad)           # 16-bit operands (the forward's image of x), fp32 partial products
    elif implicit and Cin % 64 == 0 and Cout % 4 == 0:
        dwg = hip.conv_wgrad(dz, x, k, stride, pad)                      # implicit GEMM: no im2col matrix
    else:
        kpad = wg.shape[1]
        col = hip.im2col_nhwc(x, k, k, stride, pad, kpad)
        hw = rows // n
        s1, s2 = _split(n, hw)
        part = torch.empty((s1 * s2, Cout * kpad), dtype=torch.float32, device=dev)
        ch = hw // s2                                                    # rows per partial product
        hip.gemm_ex(dz, col, part, Cout, kpad, ch, sa=(1, Cout), sb=(kpad, 1), sc=(kpad, 1), nb=(s1, s2), ba=(hw * Cout, ch * Cout),
                    bb=(hw * kpad, ch * kpad), bc=(s2 * Cout * kpad, Cout * kpad))
        dwg = hip.colsum(part, torch.zeros(Cout * kpad, dtype=torch.float32, device=dev)).view(Cout, kpad)
    if dwg is not None:
        dw = dwg[:, :k * k * Cin].reshape(Cout, k, k, Cin).permute(0, 3, 1, 2)
        if rec["sum_in"]:
            dw = dw.expand(Cout, conv.weight.shape[1], k, k)              # w_eff = sum over the identical input channels
        G.put(conv.weight, dw.contiguous())
    if not need_dx:
        return None
    Ho, Wo = conv_out(H, k, stride, pad), conv_out(W, k, stride, pad)
    g = dz if mp is None else dz16
    if Cin < 4 and implicit:
        # the stem (one input channel after the gray fold, or three): mst_conv_dgrad_stem multiplies dz by the FORWARD's GEMM weight (the
        # identical channels' kernels summed, then rounded to the operand type) per tile and gathers the taps from LDS -- no [rows, Kpad]
        # gradient matrix, no atomics; in fp32, mixed precision and 16-bit storage alike
        del col
        wstem = (wg if wg is not None else _gemm_weight(conv, rec["sum_in"]))[:, :k * k * Cin].to(g.dtype).contiguous()
        return hip.conv_dgrad_stem(g.view(n, Ho, Wo, Cout), wstem, k, stride, pad, H, W, Cin)
    if st16 or (implicit and Cout % 16 == 0 and Cin % 4 == 0 and stride in (1, 2)):
        # d input as a convolution of dz with the flipped, transposed weight (mst_conv_dgrad): no gradient matrix, no atomics
        del col
        return hip.conv_dgrad(g.view(n, Ho, Wo, Cout), hip.conv_dgrad_weight(conv.weight, g.dtype), k, stride, pad, H, W)
    kpad = wg.shape[1]
    if col is None:
        col = torch.empty((rows, kpad), dtype=torch.float32, device=dev)
    hip.gemm_ex(dz, wg, col, rows, kpad, Cout, sa=(Cout, 1), sb=(kpad, 1), sc=(kpad, 1))      # dcol overwrites col
    dx = torch.zeros_like(x)
    return hip.col2im_nhwc(col, dx, k, k, stride, pad)


def _shortcut(y: torch.Tensor, blk, mp: Optional[torch.dtype], storage16: bool):
    """The residual operand [rows, C] of the unit that closes `blk`, and the downsample unit's record (None: the identity)."""
    rd, ds = None, blk.shortcut()
    if ds is not None:
        y, rd = _conv_bn_fwd(y, *ds, False, None, False, mp, storage16)
    return y.reshape(-1, y.shape[-1]), rd


def backbone_fwd(m, x_nhwc: torch.Tensor, sum_in: bool, mp: Optional[torch.dtype] = None, storage16: bool = False):
    """torchvision resnet{18,34,50,101,152} forward in train mode up to the pooled features [n, 512 or 2048].  storage16: every activation
    between the stem's im2col and the average pool lives in mp (max pool: mst_maxpool_nhwc16, features: mst_avgpool_nhwc16).
    sv["units"]: per unit the records of its chain in forward order, then the downsample unit's record (None: the identity)."""
    sv = {"units": [], "mp": mp, "storage": "16bit" if storage16 else "fp32"}
    y, sv["stem"] = _conv_bn_fwd(x_nhwc.contiguous(), m.conv1, m.bn1, 7, 2, 3, sum_in, None, True, mp, storage16)
    sv["pool_in"] = y
    y = hip.maxpool_nhwc(y)
    for blk in m.units():
        *inner, last = blk.chain()
        h, recs = y, []
        for c in inner:
            h, r = _conv_bn_fwd(h, *c, False, None, True, mp, storage16)
            recs.append(r)
        idt, rd = _shortcut(y, blk, mp, storage16)
        y, r = _conv_bn_fwd(h, *last, False, idt, True, mp, storage16)  # the last convolution takes the residual
        sv["units"].append((*recs, r, rd))
    sv["last"] = y
    return hip.avgpool_nhwc(y), sv


def backbone_bwd(G: _Grads, sv, dfeat: torch.Tensor, need_source: bool = False) -> Optional[torch.Tensor]:
    """Parameter gradients into G (those it needs).  need_source: the stem unit hands back the gradient of the input images [n,H,W,C]
    (mst_conv_dgrad_stem); parameter gradients are computed exactly as without it."""
    y = sv["last"]
    n, H, W, Cc = y.shape
    dy = hip.avgpool_bwd_nhwc(dfeat.contiguous(), H * W).view(n * H * W, Cc)
    for first, *later, rd in reversed(sv["units"]):
        d = _conv_bn_bwd(G, later[-1], dy, True)                          # dy now carries the ReLU mask of the block output
        for r in reversed(later[:-1]):                                    # a three-long chain: through its middle to the first one's output
            d = _conv_bn_bwd(G, r, d.view(-1, d.shape[-1]), True, False)
        if rd is not None:
            dx = _conv_bn_bwd(G, rd, dy if rd["storage16"] else dy.clone(), True)    # (the 16-bit form leaves a unit without ReLU's dy alone)
        else:
            dx = dy.view(first["x"].shape).clone()
        d1 = _conv_bn_bwd(G, first, d.view(-1, d.shape[-1]), True, False)
        hip.axpby_cols(d1.view(1, -1), dx.view(1, -1))
        dy = dx.view(-1, dx.shape[-1])
    dstem = hip.maxpool_bwd_nhwc(sv["pool_in"], dy.view(sv["units"][0][0]["x"].shape))
    return _conv_bn_bwd(G, sv["stem"], dstem.view(-1, dstem.shape[-1]), need_source, False)


# ---- whole models ------------------------------------------------------------------------------------------------------
def forward_train(model, x_nhwc: torch.Tensor, sum_in: bool, B: Optional[int], D: Optional[int], mask: Optional[torch.Tensor]):
    """B/D given: ResNetSliceTrans (features -> slice transformer -> linear); else plain ResNet (features -> fc)."""
    mode = train_mode.resolve(model)
    feat, sv = backbone_fwd(model.model, x_nhwc, sum_in, mode.mp, mode.storage16)
    sv["feat"] = feat
    if B is None:
        fc = model.model.fc
        if isinstance(fc, nn.Identity):
            return feat, sv
        return hip.gemm(feat, fc.weight.detach(), fc.bias.detach()), sv
    sv["fused"], sv["fusion"] = fusion_fwd(model, feat, B, D, model.emb_ch, SLICE_HEADS, mask)
    sv["B"], sv["D"] = B, D
    return hip.gemm(sv["fused"], model.linear.weight.detach(), model.linear.bias.detach()), sv


def _head_bwd(G: _Grads, model, sv, dout: torch.Tensor) -> torch.Tensor:
    """d logits -> d features, through `linear` and the slice fusion (ResNetSliceTrans) or through `fc` / Identity (plain ResNet)."""
    if "fusion" in sv:
        dfused = G.lin_bwd(dout, sv["fused"], model.linear)
        return fusion_bwd(G, model, sv["fusion"], dfused, sv["B"], sv["D"], model.emb_ch, SLICE_HEADS)
    fc = model.model.fc
    return dout if isinstance(fc, nn.Identity) else G.lin_bwd(dout, sv["feat"], fc)


def backward_train(model, sv, dout: torch.Tensor, needed: Optional[Set[int]] = None, need_source: bool = False):
    """-> ({id(param): grad}, d x_nhwc or None).  needed: ids of the parameters whose gradient is asked for (None: all); the products
    behind the others are skipped, so a frozen model's source-only backward is the d x chain alone."""
    G = _Grads(needed=needed)
    dx = backbone_bwd(G, sv, _head_bwd(G, model, sv, dout), need_source)
    return G.by_param, dx


class _ResNetFunction(torch.autograd.Function):
    """One autograd node for the training-mode model: inputs are the parameters and the NHWC fp32 images x_nhwc.  Its gradient goes back
    through the model's own float() / permute / reshape to the source's shape, dtype and device (torch.autograd)."""

    @staticmethod
    def forward(ctx, model, x_nhwc, sum_in, B, D, mask, *params):
        with torch.no_grad():
            out, saved = forward_train(model, x_nhwc, sum_in, B, D, mask)
        ctx.model, ctx.saved, ctx.params = model, saved, params
        return out

    @staticmethod
    def backward(ctx, dout):
        needed = {id(p) for p, need in zip(ctx.params, ctx.needs_input_grad[6:]) if need}
        need_source = bool(ctx.needs_input_grad[1])
        with torch.no_grad():
            grads, dx = backward_train(ctx.model, ctx.saved, dout.contiguous().float(), needed, need_source)
        ctx.saved = None
        return (None, dx, None, None, None, None, *route_grads(grads, ctx.params, ctx.needs_input_grad[6:]))


def forward_with_grad(model, x_nhwc, sum_in: bool, B=None, D=None, mask=None):
    model._invalidate()                                  # a training step follows: the BatchNorm-folded inference weights are stale after it
    params = fp32_device_params(model)
    return _ResNetFunction.apply(model, x_nhwc, sum_in, B, D, mask, *params)


# ---- eval mode: the gradient of a frozen model's output with respect to its input volume --------------------------------------------------
def _folded_dgrad_weight(prep, key, f, Cin: int) -> torch.Tensor:
    """The folded GEMM weight [Cout, (ky, kx, c)] re-laid as mst_conv_dgrad's operand [Cin, (ky', kx', co)] (both kernel axes flipped, what
    hip.conv_dgrad_weight builds from a [Cout, Cin, k, k] weight); cached in the prepared weights beside it, by (unit, position)."""
    cache = prep.setdefault("dgrad", {})
    if key not in cache:
        Cout, k = f.w.shape[0], f.k
        cache[key] = f.w[:, :k * k * Cin].reshape(Cout, k, k, Cin).flip(1, 2).permute(3, 1, 2, 0).reshape(Cin, k * k * Cout).contiguous()
    return cache[key]


def _folded_dgrad(prep, key, f, d: torch.Tensor, shape_in) -> torch.Tensor:
    """d of a folded convolution's output [n, Ho, Wo, Cout] -> d of its input, of shape `shape_in` (mst_conv_dgrad)."""
    _, H, W, Cin = shape_in
    return hip.conv_dgrad(d, _folded_dgrad_weight(prep, key, f, Cin), f.k, f.stride, f.pad, H, W)


def _eval_backbone_fwd(model, x_nhwc: torch.Tensor, sum_in: bool):
    """The inference walk itself (`backbone_chunk`) in fp32 on the folded weights, with a keep list per chunk of `chunk_images` images:
    every ReLU output (its mask) stays for the backward.  The features are those of the fp32 inference forward bit for bit."""
    p = model._prepare(sum_in, fp32=True)
    feats, chunks = [], []
    for i0 in range(0, x_nhwc.shape[0], model.chunk_images):
        x = x_nhwc[i0:i0 + model.chunk_images].contiguous()
        keep = []
        feats.append(hip.avgpool_nhwc(backbone_chunk(p, x, keep)))
        chunks.append((x.shape, keep))
    return (torch.cat(feats, dim=0) if len(feats) > 1 else feats[0]), {"prep": p, "chunks": chunks}


def _eval_backbone_bwd(sv, dfeat: torch.Tensor) -> torch.Tensor:
    """d features [n, C] -> d x_nhwc, walking each unit's chain in reverse: mst_act_bwd on the saved ReLU output, then mst_conv_dgrad
    with the folded weight; the shortcut sums; mst_maxpool_bwd_nhwc; the stem through mst_conv_dgrad_stem.  No parameter gradient."""
    p = sv["prep"]
    outs = []
    i0 = 0
    for (n, H, W, Cin), (y0, *units) in sv["chunks"]:
        last = units[-1][1][-1]
        hw = last.shape[1] * last.shape[2]
        dy = hip.avgpool_bwd_nhwc(dfeat[i0:i0 + n].contiguous(), hw).view(n * hw, last.shape[3])
        i0 += n
        for bi in reversed(range(len(units))):
            shape_in, acts = units[bi]
            chain, ds = p["blocks"][bi]["chain"], p["blocks"][bi]["ds"]
            ins = [shape_in] + [a.shape for a in acts[:-1]]  # the input shape of every convolution of the chain
            hip.act_bwd(acts[-1], dy, 1)
            dy4 = d = dy.view(acts[-1].shape)
            for ci in reversed(range(len(chain))):
                if ci < len(chain) - 1:
                    hip.act_bwd(acts[ci], d, 1)
                d = _folded_dgrad(p, (bi, ci), chain[ci], d, ins[ci])
            # the shortcut: through the downsample, or the masked dy itself
            hip.axpby_cols((dy if ds is None else _folded_dgrad(p, (bi, "ds"), ds, dy4, shape_in)).view(1, -1), d.view(1, -1))
            dy = d.view(-1, shape_in[3])
        st = p["stem"]
        dstem = hip.maxpool_bwd_nhwc(y0, dy.view(units[0][0]))
        hip.act_bwd(y0, dstem, 1)
        outs.append(hip.conv_dgrad_stem(dstem, st.w[:, :st.k * st.k * Cin].contiguous(), st.k, st.stride, st.pad, H, W, Cin))
    return torch.cat(outs, dim=0) if len(outs) > 1 else outs[0]


class _ResNetEvalFunction(torch.autograd.Function):
    """One autograd node for a FROZEN model in eval mode: the only differentiable input is x_nhwc.  The forward is the inference forward
    (eval-mode BatchNorm folded into the convolutions, `chunk_images` images at a time) in fp32 WHATEVER the model's compute_dtype is --
    the gradient path has no 16-bit operands -- with every ReLU output kept; the logits equal the fp32 torch.no_grad() forward bit for
    bit.  ResNetSliceTrans: the logits come from the inference slice fusion (mst_slice_fusion); the op-by-op fusion of the training step
    runs beside it on the same features to keep what its backward needs.  The backward is the d x chain alone: no parameter gradient."""

    @staticmethod
    def forward(ctx, model, x_nhwc, sum_in, B, D, mask):
        with torch.no_grad():
            feat, sv = _eval_backbone_fwd(model, x_nhwc, sum_in)
            sv["feat"] = feat
            if B is None:
                fc = model.model.fc
                out = feat if isinstance(fc, nn.Identity) else hip.gemm(feat, sv["prep"]["fc"][0], sv["prep"]["fc"][1], epilogue=hip.EPI_BIAS)
            else:
                out = model.fuse(feat, B, D, mask, False)
                sv["fused"], sv["fusion"] = fusion_fwd(model, feat, B, D, model.emb_ch, SLICE_HEADS, mask)
                sv["B"], sv["D"] = B, D
        ctx.model, ctx.saved = model, sv
        return out

    @staticmethod
    def backward(ctx, dout):
        with torch.no_grad():
            G = _Grads(needed=set())                         # nothing but d x
            dx = _eval_backbone_bwd(ctx.saved, _head_bwd(G, ctx.model, ctx.saved, dout.contiguous().float()))
        ctx.saved = None
        return (None, dx, None, None, None, None)


def forward_eval_with_grad(model, x_nhwc, sum_in: bool, B=None, D=None, mask=None):
    fp32_device_params(model)
    return _ResNetEvalFunction.apply(model, x_nhwc, sum_in, B, D, mask)
