"""MI355X-native ``ResNet`` / ``ResNetSliceTrans`` -- the inference path of the reference's mst/models/resnet.py:27-243
(BASELINE configs[3] names the model).

Same constructors, ``forward`` signatures, getters and ``state_dict`` keys as the reference's 2-D torchvision branch
(``self.model`` = torchvision ``resnet{18,34}`` with ``fc`` replaced: resnet.py:44-50; ``ResNetSliceTrans`` adds the Slice
Transformer with 16 heads over 512-wide slice embeddings, ``cls_token`` and ``linear``: resnet.py:146-166).  The modules below are
parameter containers; the arithmetic runs in HIP kernels through the C ABI:

  backbone   NHWC fp32 activations; every convolution behind the stem = ``mst_conv_gemm`` (implicit GEMM: the exact-fp32 MFMA GEMM
             gathering its A operand from the activation, no im2col matrix); the stem (one input channel after the gray fold) =
             ``mst_im2col_nhwc`` + ``mst_gemm``; eval-mode
             BatchNorm folded into weight and bias and ReLU / the residual add in the GEMM epilogue; ``mst_maxpool_nhwc``,
             ``mst_avgpool_nhwc``.  Gray -> RGB (``x.repeat(1, 3, ...)``, resnet.py:176) is folded into conv1 (the three input
             channels are identical, so their kernels are summed).
  units      what a residual unit IS -- its chain of convolutions, which one takes the shortcut, the downsample -- is stated once, by
             ``_Unit.chain()`` / ``_Unit.shortcut()``; ``_fold_backbone`` turns it into ``Folded`` records that carry their geometry, and
             ``backbone_chunk`` is the one walk over them: the inference forward and the eval-mode gradient forward are that function.
  fusion     ``mst_slice_fusion`` -- the kernels of DinoV2ClassifierSlice's Slice Transformer with nhead 16, E 512.

torchvision's source is not part of the reference tree: the published resnet architecture is restated, parity of
the backbone is against ``oracle/resnet_oracle.py`` (plain torch ops) and therefore UNPINNED; the fusion half is pinned by a
fixture of the reference's own ``TransformerEncoderLayer`` (tests/golden/resnet_fusion.npz).

  training   with gradients enabled in train mode the output carries one autograd node (mst/train_resnet.py): BatchNorm with batch
             statistics, convolution / pooling / slice-transformer backward in HIP kernels (BASELINE configs[3]'s step).
  d source   ``source.grad`` / ``torch.autograd.grad(logits, source)``: the training node returns the gradient of the images too (the stem's
             data gradient: ``mst_conv_dgrad_stem``); a FROZEN model whose floating source requires grad routes to the training node in
             ``.train()`` (batch statistics, as torch would; pruned to the d x chain) and to the eval node in ``.eval()`` (folded BatchNorm,
             fp32 whatever ``compute_dtype`` is: mst/train_resnet.py::_ResNetEvalFunction); ``save_attn=True`` stays on the inference path.
  Grad-CAM++ ``save_attn=True`` (resnet.py:62-118): the map of the LAST ReLU output -- the one ``get_attention_maps`` returns --
             by ``mst_gradcampp``; the maps of the earlier ReLUs, which the reference computes and never exposes, are not produced.

Bottleneck ResNets (model 50 / 101 / 152: 2048-wide slice embeddings, 16 heads of 128) run through the same kernels (round 3).
Not built (raise): the MONAI branches (3-D, and ``pretrained=False`` in the reference), parameter
gradients through eval-mode BatchNorm (trainable parameters with ``model.eval()``).  ``pretrained=True`` needs torchvision's weights (network / hub cache); when torchvision is absent the tree
is initialised like torchvision's and a warning says so -- a checkpoint's ``state_dict`` replaces it anyway.
"""
from __future__ import annotations

import math
import os
import warnings
from typing import List, NamedTuple, Optional

import torch
import torch.nn as nn

from .base_model import BasicClassifier
from .. import hip, train_mode
from .prepared import Prepared, bind_slice_fusion, run_slice_fusion

_LAYERS = {18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 6, 3], 101: [3, 4, 23, 3], 152: [3, 8, 36, 3]}
_WIDTHS = [64, 128, 256, 512]


class _P(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container: the forward runs in libmst_hip.so")


class _Conv(_P):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin, k, k))
        nn.init.kaiming_normal_(self.weight, mode="fan_out", nonlinearity="relu")      # torchvision resnet.py init


class _BN(_P):
    def __init__(self, c):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(c))
        self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer("running_mean", torch.zeros(c))
        self.register_buffer("running_var", torch.ones(c))
        self.register_buffer("num_batches_tracked", torch.tensor(0, dtype=torch.long))
        self.eps = 1e-5


class _Linear(_P):
    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin))
        self.bias = nn.Parameter(torch.zeros(cout))
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        nn.init.uniform_(self.bias, -1 / math.sqrt(cin), 1 / math.sqrt(cin))


class _Unit(_P):
    """A residual unit: a chain of convolutions, each (conv, bn, k, stride, pad) with ReLU behind its BatchNorm; the LAST one takes the
    shortcut before its ReLU.  The shortcut is the identity (None) or a 1 x 1 downsample.  Every pass over the backbone -- the weight
    fold, the inference / eval-gradient walk, the training step and their backwards -- reads the unit's structure from here."""

    def shortcut(self):
        return (self.downsample[0], self.downsample[1], 1, self.stride, 0) if hasattr(self, "downsample") else None


class _BasicBlock(_Unit):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1, self.bn1 = _Conv(cin, cout, 3), _BN(cout)
        self.conv2, self.bn2 = _Conv(cout, cout, 3), _BN(cout)
        self.stride = stride
        if stride != 1 or cin != cout:
            self.downsample = nn.ModuleList([_Conv(cin, cout, 1), _BN(cout)])       # keys downsample.0.* / downsample.1.*

    def chain(self):
        return [(self.conv1, self.bn1, 3, self.stride, 1), (self.conv2, self.bn2, 3, 1, 1)]


class _Bottleneck(_Unit):
    """torchvision Bottleneck (v1.5): 1x1 -> 3x3 (carries the stride) -> 1x1 (x4), each with its BatchNorm (models 50 / 101 / 152:
    reference resnet.py:44-50 takes whichever torchvision model `model` names; emb_ch 2048, resnet.py:152)."""

    def __init__(self, cin, w, stride):
        super().__init__()
        self.conv1, self.bn1 = _Conv(cin, w, 1), _BN(w)
        self.conv2, self.bn2 = _Conv(w, w, 3), _BN(w)
        self.conv3, self.bn3 = _Conv(w, 4 * w, 1), _BN(4 * w)
        self.stride = stride
        if stride != 1 or cin != 4 * w:
            self.downsample = nn.ModuleList([_Conv(cin, 4 * w, 1), _BN(4 * w)])

    def chain(self):
        return [(self.conv1, self.bn1, 1, 1, 0), (self.conv2, self.bn2, 3, self.stride, 1), (self.conv3, self.bn3, 1, 1, 0)]


class _TVResNet(_P):
    """Parameter tree of torchvision.models.resnet{18,34,50,101,152} (keys conv1, bn1, layer1..4.<i>.*, fc)."""

    def __init__(self, model: int, fc_out: Optional[int]):
        super().__init__()
        if model not in _LAYERS:
            raise NotImplementedError(f"resnet{model}: torchvision's resnet 18 / 34 / 50 / 101 / 152 are built on the HIP path")
        self.conv1, self.bn1 = _Conv(3, 64, 7), _BN(64)
        cin = 64
        for li, (n, w) in enumerate(zip(_LAYERS[model], _WIDTHS)):
            blocks = []
            for b in range(n):
                stride = 2 if (b == 0 and li > 0) else 1
                if model >= 50:
                    blocks.append(_Bottleneck(cin, w, stride))
                    cin = 4 * w
                else:
                    blocks.append(_BasicBlock(cin, w, stride))
                    cin = w
            setattr(self, f"layer{li + 1}", nn.ModuleList(blocks))
        self.out_features = cin
        self.fc = nn.Identity() if fc_out is None else _Linear(cin, fc_out)

    def units(self):                                     # in forward order
        return [blk for li in range(4) for blk in getattr(self, f"layer{li + 1}")]


def conv_out(size: int, k: int, stride: int, pad: int) -> int:
    """Output extent of a convolution (or pooling window) along one axis."""
    return (size + 2 * pad - k) // stride + 1


def _conv(x: torch.Tensor, w: torch.Tensor, b, k: int, stride: int, pad: int, kpad: int, epilogue: int, out=None) -> torch.Tensor:
    """One convolution of the backbone on an NHWC activation -> [n*Ho*Wo, Cout]: the implicit GEMM (mst_conv_gemm) when the input
    channels allow it (Cin % 16 == 0: every layer behind the stem) and there are more than 1,024 output pixels, else im2col + GEMM.  MST_CONV_IM2COL=1 forces the latter (A/B)."""
    n, H, W, cin = x.shape
    if x.dtype != torch.float32:                         # compute_dtype bf16 / fp16: the implicit GEMM on 16-bit MFMA operands (Cin % 64 == 0)
        return hip.conv_gemm16(x, w, b, k, k, stride, pad, epilogue=epilogue, out=out)
    rows = n * conv_out(H, k, stride, pad) * conv_out(W, k, stride, pad)
    # up to 1,024 output pixels mst_gemm has its 32 x 32-tile kernel (k_gemm32s.hip), which fills the chip where 128 x 128 tiles cannot
    if cin % 16 == 0 and rows > 1024 and os.environ.get("MST_CONV_IM2COL", "0") != "1":
        return hip.conv_gemm(x, w, b, k, k, stride, pad, epilogue=epilogue, out=out)
    return hip.gemm(hip.im2col_nhwc(x, k, k, stride, pad, kpad), w, b, epilogue=epilogue, out=out)


class Folded(NamedTuple):
    """One convolution with its eval-mode BatchNorm folded in: the GEMM operands and the geometry every walk needs."""
    w: torch.Tensor
    b: torch.Tensor
    kpad: int
    k: int
    stride: int
    pad: int


def _fold(conv: _Conv, bn: _BN, k: int, stride: int, pad: int, sum_in: bool, dev, dtype: torch.dtype = torch.float32, kmul: int = 16) -> Folded:
    """Eval-mode BatchNorm folded into the convolution: GEMM weight [Cout, Kpad] in (ky, kx, c) order (fp32, or rounded to the 16-bit
    compute type AFTER the fold) + bias [Cout] fp32; K padded to a multiple of kmul."""
    w = conv.weight.detach().to(dev, torch.float32)
    if sum_in:
        w = w.sum(dim=1, keepdim=True)                   # identical input channels (gray -> RGB repeat): one summed kernel
    s = bn.weight.detach().to(dev, torch.float32) / torch.sqrt(bn.running_var.to(dev, torch.float32) + bn.eps)
    b = bn.bias.detach().to(dev, torch.float32) - bn.running_mean.to(dev, torch.float32) * s
    w = (w * s[:, None, None, None]).permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    K = w.shape[1]
    kpad = (K + kmul - 1) // kmul * kmul
    if kpad != K:
        w = torch.cat([w, w.new_zeros(w.shape[0], kpad - K)], dim=1)
    return Folded(w.to(dtype).contiguous(), b.contiguous(), kpad, k, stride, pad)


def _conv_folded(x: torch.Tensor, f: Folded, epilogue: int, out=None) -> torch.Tensor:
    """`_conv` of a folded record -> NHWC [n, Ho, Wo, Cout] (a view of `out` when one is given)."""
    n, H, W, _ = x.shape
    y = _conv(x, f.w, f.b, f.k, f.stride, f.pad, f.kpad, epilogue, out)
    return y.view(n, conv_out(H, f.k, f.stride, f.pad), conv_out(W, f.k, f.stride, f.pad), f.w.shape[0])


def backbone_chunk(p, x: torch.Tensor, keep: Optional[list] = None) -> torch.Tensor:
    """Stem, max pool and every residual unit for one chunk of images [n, H, W, C] fp32 on the prepared weights `p` -> the last ReLU
    output [n, h, w, C'] in p's activation type.  The ONE walk over the folded backbone: the inference forward (`ResNet._features`) and
    the eval-mode gradient node (mst/train_resnet.py) both run it, so their bits cannot drift apart.

    keep None: relu(identity + .) of a unit without downsample is formed in place on the unit's input, which is dead after it, and
    nothing outlives its last reader.  keep a list: the backward needs every ReLU output (its mask), so that sum goes into a copy -- the
    same kernels on the same operands -- and keep receives the stem's output before the pool, then per unit (input shape, [the ReLU
    outputs in chain order, the unit's output last])."""
    st = p["stem"]
    if p["dtype"] == torch.float32:
        y = _conv_folded(x, st, hip.EPI_BIAS_RELU)       # Cin 1 or 3: mst_im2col_nhwc + mst_gemm
    else:
        # the stem's 49 taps of ONE input channel are no multiple of 64 channels: its im2col rows (padded to 64, rounded on the way out)
        # are the "pixels" of a 1 x 1 convolution; everything behind it, the max pool included, is 16-bit
        n, H, W, _ = x.shape
        Ho, Wo = conv_out(H, st.k, st.stride, st.pad), conv_out(W, st.k, st.stride, st.pad)
        col = hip.im2col_nhwc(x, st.k, st.k, st.stride, st.pad, st.kpad, out_dtype=p["dtype"]).view(n, Ho, Wo, st.kpad)
        y = hip.conv_gemm16(col, st.w, st.b, 1, 1, 1, 0, epilogue=hip.EPI_BIAS_RELU).view(n, Ho, Wo, 64)
        del col
    if keep is not None:
        keep.append(y)
    y = hip.maxpool_nhwc(y)
    for u in p["blocks"]:
        h, acts = y, []
        for f in u["chain"][:-1]:
            h = _conv_folded(h, f, hip.EPI_BIAS_RELU)
            if keep is not None:
                acts.append(h)
        if u["ds"] is not None:
            idt = _conv_folded(y, u["ds"], hip.EPI_BIAS)
        else:
            idt = y if keep is None else y.clone()       # y carries the previous unit's ReLU mask: a backward still reads it
        shape_in = y.shape
        y = _conv_folded(h, u["chain"][-1], hip.EPI_RESIDUAL_RELU, out=idt.view(-1, idt.shape[-1]))     # relu(identity + bn(conv(.)))
        if keep is not None:
            keep.append((shape_in, acts + [y]))
    return y


class ResNet(BasicClassifier):
    def __init__(self, in_ch, out_ch, spatial_dims=3, model=34, pretrained=False, kwargs_resnet={}, **kwargs):
        emb_ch = kwargs.pop("emb_ch", out_ch)
        self.chunk_images = int(kwargs.pop("chunk_images", 128))      # build-specific: images per backbone pass (activation memory:
        #                                                               0.4 GB for the stem's output at 128 images of 224 x 224)
        # build-specific: MFMA operand / activation type of the INFERENCE backbone: 'fp32' (default, exact: the parity mode) | 'bf16' | 'fp16'
        # (16-bit NHWC activations behind the stem's max pool, fp32 accumulation, folded BatchNorm bias in fp32; the slice transformer and
        # the head stay fp32).  The training step is fp32 whatever this says.
        cdt = str(kwargs.pop("compute_dtype", os.environ.get("MST_RESNET_DTYPE", "fp32"))).lower()
        if cdt not in ("fp32", "bf16", "fp16"):
            raise ValueError("ResNet: compute_dtype must be 'fp32', 'bf16' or 'fp16'")
        self.compute_dtype_name = cdt
        # build-specific: the training mode (mst/train_mode.py): train_precision and train_storage; a ResNet has no train_attention, and
        # DinoV2ClassifierSlice's MST_TRAIN_STORAGE does not reach it
        tp, _, ts, precision_given = train_mode.from_kwargs(kwargs, storage_env="MST_RESNET_TRAIN_STORAGE", attention=False)
        self.train_precision = tp
        self.train_storage = ts
        self._train_precision_given = precision_given
        super().__init__(in_ch, out_ch, spatial_dims, **kwargs)
        self.attention_maps = []
        if spatial_dims != 2:
            raise NotImplementedError("ResNet: only the 2-D (torchvision) branch of the reference is built on the HIP path; the 3-D "
                                      "MONAI branch is not (SURVEY.md 8f-2)")
        fc_out = None if emb_ch is None else emb_ch
        self.model = _TVResNet(model, fc_out)
        if pretrained:
            try:                                         # reference resnet.py:44-45: torchvision weights="DEFAULT" (network / hub cache)
                import torchvision.models as tvm
                tv = getattr(tvm, f"resnet{model}")(weights="DEFAULT")
                sd = {k: v for k, v in tv.state_dict().items() if not k.startswith("fc.") or (emb_ch == 1000)}
                self.model.load_state_dict(sd, strict=False)
            except Exception as e:  # pragma: no cover - torchvision is not in this image
                warnings.warn(f"ResNet(pretrained=True): torchvision weights unavailable ({type(e).__name__}); the backbone keeps "
                              "torchvision's random initialisation until a checkpoint is loaded")
        else:
            warnings.warn("ResNet(pretrained=False): the reference builds a MONAI resnet here; this build keeps the torchvision "
                          "parameter layout with torchvision's initialisation")
        # device-side weight images, keyed on every parameter AND BatchNorm buffer: an optimiser step, a running-statistics update
        # or any weight surgery makes them stale (an eval forward after training steps reused the first eval's fold)
        self._prepared = Prepared()
        self.register_load_state_dict_post_hook(lambda module, incompatible: module._invalidate())

    def _invalidate(self):
        self._prepared.invalidate()

    def _apply(self, fn, *args, **kwargs):
        self._invalidate()
        return super()._apply(fn, *args, **kwargs)

    # ---- backbone -------------------------------------------------------------------------------------------------------
    def _prepare(self, sum_in: bool, fp32: bool = False):
        """The BatchNorm-folded weights in compute_dtype.  fp32: in fp32 whatever compute_dtype is -- what the eval-mode gradient
        node runs on; the same image when compute_dtype is fp32, one of its own beside it otherwise."""
        name = "fp32" if fp32 else self.compute_dtype_name
        return self._prepared.get(self, "backbone_" + name, lambda: self._fold_backbone(sum_in, name), sum_in, str(self.device), name)

    def _fold_backbone(self, sum_in: bool, name: str):
        cdt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[name]
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(f"ResNet runs on an MI355X only: parameters are on {dev}; call .to('cuda'). There is no CPU fallback.")
        m = self.model
        # 16-bit: the stem's im2col rows are padded to 64 columns so that they are one "pixel" of a 1 x 1 convolution for mst_conv_gemm16
        prep = {"dtype": cdt, "stem": _fold(m.conv1, m.bn1, 7, 2, 3, sum_in, dev, cdt, 16 if cdt == torch.float32 else 64), "blocks": []}
        for blk in m.units():
            ds = blk.shortcut()
            prep["blocks"].append({"chain": [_fold(*c, False, dev, cdt) for c in blk.chain()],
                                   "ds": None if ds is None else _fold(*ds, False, dev, cdt)})
        if not isinstance(m.fc, nn.Identity):
            prep["fc"] = (m.fc.weight.detach().to(dev, torch.float32).contiguous(), m.fc.bias.detach().to(dev, torch.float32).contiguous())
        return prep

    def _features(self, x_nhwc: torch.Tensor, sum_in: bool, keep_last: bool = False) -> torch.Tensor:
        """[n, H, W, C] fp32 on the device -> [n, 512] (avgpool output, before fc).  keep_last: the last ReLU output of every image
        stays in ``self._last_act`` [n, h*w, 512] for Grad-CAM++."""
        p = self._prepare(sum_in)
        outs: List[torch.Tensor] = []
        lasts: List[torch.Tensor] = []
        for i0 in range(0, x_nhwc.shape[0], self.chunk_images):
            x = x_nhwc[i0:i0 + self.chunk_images].contiguous()
            y = backbone_chunk(p, x)
            if y.dtype != torch.float32:
                y = hip.cvt32(y)                         # the average pool and Grad-CAM++ read fp32
            outs.append(hip.avgpool_nhwc(y))
            if keep_last:
                lasts.append(y)
        if keep_last:
            y = torch.cat(lasts, dim=0) if len(lasts) > 1 else lasts[0]
            self._last_hw = (y.shape[1], y.shape[2])
            self._last_act = y.view(y.shape[0], -1, y.shape[3])
        return torch.cat(outs, dim=0) if len(outs) > 1 else outs[0]

    def _wants_grad(self) -> bool:
        if not torch.is_grad_enabled() or not any(p.requires_grad for p in self.parameters()):
            return False
        if not self.training:
            raise NotImplementedError("ResNet: gradients through eval-mode BatchNorm are not on the HIP path; call .train() for a "
                                      "training step or run the forward under torch.no_grad()")
        return True

    def _source_grad_route(self, x: torch.Tensor, save_attn: bool) -> Optional[str]:
        """No parameter requires grad (``_wants_grad`` was False): does the SOURCE ask for a gradient?  'train' (.train(): the training
        node with batch statistics, as torch would, pruned to the d x chain), 'eval' (.eval(): the frozen-model node on the folded
        BatchNorm, mst/train_resnet.py::_ResNetEvalFunction) or None: the inference path -- also for ``save_attn=True``, whose Grad-CAM++
        maps come from the inference forward."""
        if save_attn or not torch.is_grad_enabled() or not (x.is_floating_point() and x.requires_grad):
            return None
        return "train" if self.training else "eval"

    def _gradcam(self, out: torch.Tensor, fc_weight: Optional[torch.Tensor]):
        """resnet.py:66-70 + 93-118 for the last ReLU: attention_maps[-1] = [N, 1, h, w]."""
        h, w = self._last_hw
        cam = hip.gradcampp(self._last_act, out.detach().contiguous(), fc_weight)
        self.attention_maps = [cam.view(-1, 1, h, w)]
        self._last_act = None

    def forward(self, source, save_attn=False, **kwargs):
        x = source.to(self.device)                       # [N, C, H, W]
        if x.dim() != 4:
            raise RuntimeError(f"Expected 4D input [N, C, H, W] to the 2-D resnet, got {tuple(x.shape)}")
        if x.shape[1] != 3:
            raise RuntimeError(f"Given groups=1, weight of size [64, 3, 7, 7], expected input{list(x.shape)} to have 3 channels, "
                               f"but got {x.shape[1]} channels instead")
        x = x.float().permute(0, 2, 3, 1).contiguous()
        if self._wants_grad():
            if save_attn:
                raise NotImplementedError("ResNet: save_attn inside a training forward is not supported; compute the maps under "
                                          "torch.no_grad()")
            from .. import train_resnet
            return train_resnet.forward_with_grad(self, x, False)
        route = self._source_grad_route(x, save_attn)
        if route is not None:                            # a frozen model, a source that requires grad: d logits / d source
            from .. import train_resnet
            return (train_resnet.forward_with_grad if route == "train" else train_resnet.forward_eval_with_grad)(self, x, False)
        feat = self._features(x, False, keep_last=save_attn)
        p = self._prepare(False)
        out = hip.gemm(feat, p["fc"][0], p["fc"][1], epilogue=hip.EPI_BIAS) if "fc" in p else feat
        if save_attn:
            self._gradcam(out, p["fc"][0] if "fc" in p else None)
        return out

    def get_attention_maps(self):
        return self.attention_maps[-1]                   # [N, 1, h, w]  (resnet.py:75-76)


SLICE_HEADS = 16      # reference resnet.py:151


class _SliceLayer(_P):
    def __init__(self, E):
        super().__init__()
        holder = _P()
        holder.in_proj_weight = nn.Parameter(torch.empty(3 * E, E))
        holder.in_proj_bias = nn.Parameter(torch.zeros(3 * E))
        holder.out_proj = _Linear(E, E)
        nn.init.xavier_uniform_(holder.in_proj_weight)
        nn.init.zeros_(holder.out_proj.bias)
        self.self_attn = holder
        self.linear1, self.linear2 = _Linear(E, E), _Linear(E, E)
        self.norm1, self.norm2 = _LN(E), _LN(E)


class _LN(_P):
    def __init__(self, E):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(E))
        self.bias = nn.Parameter(torch.zeros(E))


class _SliceFusion(_P):
    def __init__(self, E):
        super().__init__()
        self.layers = nn.ModuleList([_SliceLayer(E)])
        self.norm = _LN(E)


class ResNetSliceTrans(ResNet):
    def __init__(self, in_ch, out_ch, spatial_dims=2, model=34, pretrained=True, kwargs_resnet={},
                 rotary_positional_encoding=None, optimizer_kwargs={"lr": 1e-5, "weight_decay": 1e-2}, **kwargs):
        super().__init__(in_ch, out_ch, spatial_dims, emb_ch=None, model=model, pretrained=pretrained, kwargs_resnet=kwargs_resnet,
                         optimizer_kwargs=optimizer_kwargs, **kwargs)
        if rotary_positional_encoding is not None:
            raise NotImplementedError("ResNetSliceTrans: rotary variants are wired for DinoV2ClassifierSlice only")
        emb_ch = 512 if model <= 34 else 2048
        self.emb_ch = emb_ch
        self.attention_maps_slice = []
        self.slice_fusion = _SliceFusion(emb_ch)
        self.cls_token = nn.Parameter(torch.randn(1, 1, emb_ch))
        self.linear = _Linear(emb_ch, out_ch)
        self._ws = {}

    def _fusion_weights(self):
        dev = self.device
        keep = []                                        # (copies exist only where a parameter is not already fp32 on the device)

        def f32(t):
            t = t.detach().to(dev, torch.float32).contiguous()
            keep.append(t)
            return t

        fw = hip.FusionWeights()
        fw.emb_in = fw.emb = fw.head_in = self.emb_ch
        fw.num_heads, fw.fusion_type, fw.out_ch = SLICE_HEADS, hip.FUSION_TRANSFORMER, self.out_ch
        bind_slice_fusion(fw, self.slice_fusion, self.cls_token, f32)
        fw.head_w, fw.head_b = hip.ptr(f32(self.linear.weight)), hip.ptr(f32(self.linear.bias))
        return fw, keep

    def fuse(self, emb: torch.Tensor, B: int, D: int, src_key_padding_mask=None, save_attn: bool = False) -> torch.Tensor:
        """[B*D, 512] slice embeddings -> logits [B, out_ch] (resnet.py:180-191)."""
        fw, _ = self._prepared.get(self, "fusion", self._fusion_weights)
        _, logits, probs = run_slice_fusion(fw, emb, B, D, src_key_padding_mask, True, save_attn, self._ws)
        if save_attn:
            self.attention_maps_slice = [probs]
        return logits

    def forward(self, source, src_key_padding_mask=None, **kwargs):
        save_attn = bool(kwargs.get("save_attn"))
        x = source.to(self.device)                       # [B, C, D, H, W]
        B, C, D, H, W = x.shape
        if C != 1:                                       # x.repeat(1, 3, ...) then a 3-channel conv1: only gray volumes fit (resnet.py:176)
            raise RuntimeError(f"Given groups=1, weight of size [64, 3, 7, 7], expected input[{B * D}, {3 * C}, {H}, {W}] to have 3 "
                               f"channels, but got {3 * C} channels instead")
        self._last_shape = (B, D)
        x = x.float().reshape(B * D, H, W, 1).contiguous()                              # 'b c d h w -> (b d) c h w', gray -> RGB folded
        if self._wants_grad():
            if save_attn:
                raise NotImplementedError("ResNetSliceTrans: save_attn inside a training forward is not supported; compute the maps "
                                          "under torch.no_grad()")
            from .. import train_resnet
            return train_resnet.forward_with_grad(self, x, True, B, D, src_key_padding_mask)
        route = self._source_grad_route(x, save_attn)
        if route is not None:                            # a frozen model, a source that requires grad: d logits / d source
            from .. import train_resnet
            fwd = train_resnet.forward_with_grad if route == "train" else train_resnet.forward_eval_with_grad
            return fwd(self, x, True, B, D, src_key_padding_mask)
        emb = self._features(x, True, keep_last=save_attn)
        if save_attn:
            self._gradcam(emb, None)                     # super().forward(x, save_attn=True) with fc = Identity (resnet.py:181)
        return self.fuse(emb, B, D, src_key_padding_mask, save_attn)

    def get_slice_attention(self):
        B, D = self._last_shape
        sp = self.attention_maps_slice[-1].contiguous()                              # [B, heads, 1+D, 1+D]
        out = torch.empty((B * D,), dtype=torch.float32, device=sp.device)
        hip.attention_readout(None, sp, B, D, 1, 2, 0, SLICE_HEADS, None, out, None)
        return out[:, None, None]                        # [B*D, 1, 1]  (resnet.py:196-205)

    def get_attention_maps(self):
        return self.get_slice_attention().unsqueeze(-1) * super().get_attention_maps()      # [B*D, 1, h, w]  (resnet.py:207-212)
