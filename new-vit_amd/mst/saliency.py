"""Device-side `--get_attention` post-processing: a drop-in for ``run_pred`` of the reference's scripts/main_predict.py
(l.134-165) when the model is this package's DinoV2ClassifierSlice.

The reference runs, per volume and per test-time-augmentation flip, the forward, three getters, a head mean, flips and at
the end ``F.interpolate(..., mode='trilinear')`` as separate torch ops on [1,1,D,H,W] tensors.  Here the forward is the HIP
path and everything after it is two kernels of libmst_hip (mst_saliency_accumulate at the patch-grid resolution, ONE
mst_saliency_upsample); torch only flips the input volume and expands the per-slice vector (views, no arithmetic).

Test-time augmentation (l.147-158) also has a folded form, ``run_pred(..., use_tta=True, tta="folded")``: the four in-plane flips in
one encoder pass (mst_tta_inplane_flips), the four depth flips as reversed slice orders in front of the slice transformer, one
mst_saliency_accumulate_tta launch.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import hip
from .models.dino import SLICE_HEADS, DinoV2ClassifierSlice

TTA_FLIPS = [(2,), (3,), (4,), (2, 3), (2, 4), (3, 4), (2, 3, 4)]     # scripts/main_predict.py:148


TTA_MASKS = [0] + [sum(1 << (a - 2) for a in dims) for dims in TTA_FLIPS]   # bit 0 depth, bit 1 height, bit 2 width
TTA_MODES = ("loop", "folded")


def run_pred(model, batch, save_attn: bool = False, use_softmax: bool = True, use_tta: bool = False, tta: str = "loop"
             ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """(pred [B,out], weight [1,1,D,H,W] | None, weight_slice [1,1,D,H,W] | None) exactly as the script's run_pred.

    ``tta`` chooses how ``use_tta=True`` computes its eight variants (without ``use_tta`` it has no effect):
      "loop"    eight forwards of the flipped volume, one after the other, as the script does (the default);
      "folded"  the same three results from ONE encoder pass: the encoder is per slice, so a flip along D only reorders slice
                embeddings and CLS attention rows, and the eight variants are the four in-plane flips (mst_tta_inplane_flips, 4*B*D
                slices in one ``encode_slices`` call) each fused twice, once with the slice order reversed (one ``fuse_slices`` call on
                8*B volumes; the padding mask is repeated unflipped, as the script passes it).  The saliency is one
                mst_saliency_accumulate_tta launch (fixed summation order: two calls give the same bits) and one up-sampling.  This
                mode neither fills nor reads ``model.attention_maps`` / ``attention_maps_slice`` / ``_cls_last`` (the getters keep
                answering for the last ``forward``), and it refuses a model whose slices are sharded over several ranks, because
                it calls ``encode_slices`` directly."""
    if not isinstance(model, DinoV2ClassifierSlice):
        raise TypeError("mst.saliency.run_pred drives this package's DinoV2ClassifierSlice only")
    if tta not in TTA_MODES:
        raise ValueError(f"tta must be 'loop' or 'folded', got {tta!r}")
    folded = bool(use_tta) and tta == "folded"
    if folded and model._sharding is not None and model._sharding.world_size > 1:
        raise NotImplementedError("tta='folded' calls encode_slices directly and does not shard the slices over ranks: "
                                  "use tta='loop' under slice sharding")
    source, mask = batch["source"], batch.get("src_key_padding_mask", None)
    source = source.to(model.device)
    if save_attn and source.shape[0] != 1:
        raise RuntimeError(f"shape '[1, 1, {source.shape[2]}, ...]' is invalid for a batch of {source.shape[0]} volumes "
                           "(main_predict.py:98 views the maps as one volume)")
    if folded:
        return _run_pred_folded(model, source, mask, save_attn, use_softmax)
    D, H, W = (int(v) for v in source.shape[2:])
    low = ws = None
    pred = None
    flips = [()] + (TTA_FLIPS if use_tta else [])
    for dims in flips:
        src = torch.flip(source, dims) if dims else source
        with torch.no_grad():
            p = model(src, src_key_padding_mask=mask, save_attn=save_attn)
        if use_softmax:
            p = torch.softmax(p, dim=-1)                    # l.63-64
        pred = p if pred is None else pred + p
        if save_attn:
            maps = model.get_attention_maps()              # [D, heads, Np]
            sa = model.get_slice_attention().reshape(-1)    # [D]
            g = int(maps.shape[-1] ** 0.5)                  # l.91: square patch grid assumed by the script
            if low is None:
                low = torch.empty((D, g, g), dtype=torch.float32, device=maps.device)
                ws = torch.empty((D,), dtype=torch.float32, device=maps.device)
            fm = sum(1 << (a - 2) for a in dims)
            hip.saliency_accumulate(maps.contiguous(), sa.contiguous(), g, g, fm, low, ws, accumulate=bool(dims))
    n = float(len(flips))
    pred = pred / n if use_tta else pred
    if not save_attn:
        return pred, None, None
    weight = hip.saliency_upsample(low, (D, H, W), scale=1.0 / n)[None, None]            # l.155-163
    weight_slice = (ws / n).view(1, 1, D, 1, 1).expand(1, 1, D, H, W)                     # l.102-103, 156
    return pred, weight, weight_slice


def _run_pred_folded(model, source, mask, save_attn: bool, use_softmax: bool):
    """run_pred(use_tta=True) with the depth flips folded out of the encoder; variant v of TTA_MASKS is the in-plane flip
    TTA_MASKS[v] >> 1 (rows f*B*D .. of the one encoder call) with the D axis reversed when TTA_MASKS[v] & 1."""
    B, C, D, H, W = (int(v) for v in source.shape)
    if C != 1:
        raise NotImplementedError("tta='folded' takes one-channel volumes [B, 1, D, H, W] (channels become slices that a depth flip "
                                  "does not reverse): use tta='loop'")
    if save_attn and model.slice_fusion_type != "transformer":
        raise RuntimeError(f"save_attn needs the slice transformer's attention; slice_fusion is {model.slice_fusion_type!r}")
    x = source if source.dtype in (torch.float32, torch.float16, torch.bfloat16) else source.float()
    enc = model.encoder
    with torch.no_grad():
        slices = hip.tta_inplane_flips(x.reshape(B * D, H, W).contiguous())                       # [4, B*D, H, W]
        emb, cls_probs, _ = model.encode_slices(slices.view(4 * B * D, H, W), enc.depth if save_attn else 0, False)
        emb = emb.view(4, B, D, -1)
        rev = emb.flip(2)
        variants = torch.stack([(rev if m & 1 else emb)[m >> 1] for m in TTA_MASKS])              # [8, B, D, E]
        mask8 = None if mask is None else mask.to(model.device).repeat(8, 1)                      # l.149: the mask is NOT flipped
        want_logits = not isinstance(model.linear, torch.nn.Identity)
        features, logits, slice_probs = model.fuse_slices(variants.view(8 * B * D, -1), 8 * B, D, mask8, bool(save_attn), want_logits)
        p = (logits if want_logits else features).view(8, B, -1)
        if use_softmax:
            p = torch.softmax(p, dim=-1)                    # l.63-64
        pred = p[0]
        for v in range(1, 8):                               # the loop's order of additions
            pred = pred + p[v]
        pred = pred / 8.0
        if not save_attn:
            return pred, None, None
        heads, N = int(cls_probs.shape[2]), int(cls_probs.shape[3])
        R = 4 if model.use_registers else 0                 # img_slice = slice(5, None): dino.py:191
        Np = N - 1 - R
        dev = emb.device
        plane = torch.empty((4, D, heads, Np), dtype=torch.float32, device=dev)
        hip.attention_readout(cls_probs[-1].contiguous(), None, 4, D, heads, N, R, SLICE_HEADS, plane, None, None)
        sa = torch.empty((8, D), dtype=torch.float32, device=dev)
        hip.attention_readout(None, slice_probs.contiguous(), 8, D, 1, 2, 0, SLICE_HEADS, None, sa, None)
        g = int(Np ** 0.5)                                  # l.91: square patch grid assumed by the script
        low = torch.empty((D, g, g), dtype=torch.float32, device=dev)
        ws = torch.empty((D,), dtype=torch.float32, device=dev)
        hip.saliency_accumulate_tta(plane, sa, g, g, low, ws)
        weight = hip.saliency_upsample(low, (D, H, W), scale=1.0 / 8)[None, None]                 # l.155-163
    weight_slice = (ws / 8.0).view(1, 1, D, 1, 1).expand(1, 1, D, H, W)                           # l.102-103, 156
    return pred, weight, weight_slice
