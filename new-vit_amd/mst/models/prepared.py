"""What the three model classes share about their device-side weight images (packed, folded, cast, or bound into a C struct):

  version_key / Prepared   WHEN an image is stale: one identity of a list of tensors, one holder of the images built from it.
  bind_slice_fusion        the Slice Transformer's parameters -> the fields of ``mst_fusion_weights`` (include/mst_hip.h).
  run_slice_fusion         the one call of ``mst_slice_fusion``: outputs, mask, workspace.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import torch

from .. import hip


def version_key(tensors, full: bool) -> tuple:
    """Identity of `tensors` (parameters and buffers alike) as far as an in-place edit or a replaced storage can change it.
    full: every tensor's (data_ptr, _version) pair -- what a training loop wants, whose optimiser rewrites parameters in place.
    Otherwise ONE pass folding the whole pointer and the version of every tensor in order, plus the count (~15 us for ~200 tensors
    where the tuple of pairs costs ~50 us, 5 % of a 1.1 ms forward).  Either form changes with an edit of ANY one tensor, tells
    WHICH tensor of the list was edited, and keeps all pointer bits: a sum of versions and low pointer bits does none of the three."""
    if full:
        return tuple((t.data_ptr(), t._version) for t in tensors)
    acc = 0
    for t in tensors:
        acc = (acc * 1000003 + t._version + t.data_ptr()) & 0xFFFFFFFFFFFFFFFF
    return (acc, len(tensors))


class Prepared:
    """The images one model built from its parameters and buffers, by name, each with the key it was built under.  The tensor list is
    read off the module once, then cached: ``invalidate`` after anything that REPLACES a tensor -- ``_apply``, ``load_state_dict`` -- or
    that writes one behind the version counters: a ``.data`` view, a kernel handed a raw pointer.  The module is an argument, not a
    member: a holder that pointed back at its owner would leave the model's device memory to the cycle collector."""

    def __init__(self):
        self._tensors = None
        self._slots: Dict[str, tuple] = {}

    def invalidate(self):
        self._tensors = None
        self._slots.clear()

    def __deepcopy__(self, memo):
        """A copied model builds its own images from its own parameters (the slots hold C structs of raw pointers into this one's)."""
        return Prepared()

    def key(self, module: torch.nn.Module, full: bool, *extra) -> tuple:
        """`extra` (whatever else the image depends on), then version_key of the module's tensors."""
        if self._tensors is None:
            self._tensors = [*module.parameters(), *module.buffers()]
        return extra + version_key(self._tensors, full)

    def get(self, module: torch.nn.Module, name: str, build: Callable[[], object], *extra):
        """The image `name`, built by `build()` when there is none for the current key.  Both forms of the key are stored with it:
        the form read follows ``torch.is_grad_enabled()``."""
        full = torch.is_grad_enabled()
        slot = self._slots.get(name)
        if slot is not None and slot[0][full] == self.key(module, full, *extra):
            return slot[1]
        value = build()
        self._slots[name] = ({True: self.key(module, True, *extra), False: self.key(module, False, *extra)}, value)
        return value


def cached_workspace(cache: dict, name: str, nbytes: int, dev) -> torch.Tensor:
    """cache[name]: device scratch of at least `nbytes` bytes on `dev`, kept from call to call and grown on demand."""
    t = cache.get(name)
    if t is None or t.numel() < nbytes or t.device != dev:
        t = cache[name] = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return t


def pin_workspaces(entry: dict, cache: dict) -> dict:
    """A captured graph replays raw pointers into the workspaces of `cache` as they were when it was captured, and cached_workspace
    REPLACES a tensor as soon as a larger shape arrives.  So the graph's entry takes a reference to every workspace tensor live at its
    capture: a replaced workspace then stays allocated (the caching allocator cannot hand its memory to anyone else) for exactly as
    long as the graph that writes into it, and a replay of an earlier, smaller shape keeps working in its own scratch.  Dropping the
    graphs on growth instead would recapture (two eager calls and a capture per key) every time a batch alternates between volumes of
    different depth.  Needs no device: `entry` is any dict, the tensors may live anywhere.  Returns the entry."""
    entry["ws"] = dict(cache)
    return entry


def bind_slice_fusion(fw: hip.FusionWeights, slice_fusion, cls_token: torch.Tensor, f32: Callable[[torch.Tensor], torch.Tensor]):
    """nn.TransformerEncoder(num_layers=1, norm=LayerNorm) + the class token -> fw's transformer fields.  `f32` hands back the fp32
    device image of a parameter and keeps it alive.  Everything else of fw (sizes, bottleneck, slice_pos_emb, rotary tables, the
    head) is its model's."""
    lay = slice_fusion.layers[0]
    attn = lay.self_attn
    for field, t in (("cls_token", cls_token.reshape(-1)),
                     ("ln1_w", lay.norm1.weight), ("ln1_b", lay.norm1.bias),
                     ("in_proj_w", attn.in_proj_weight), ("in_proj_b", attn.in_proj_bias),
                     ("out_proj_w", attn.out_proj.weight), ("out_proj_b", attn.out_proj.bias),
                     ("ln2_w", lay.norm2.weight), ("ln2_b", lay.norm2.bias),
                     ("lin1_w", lay.linear1.weight), ("lin1_b", lay.linear1.bias),
                     ("lin2_w", lay.linear2.weight), ("lin2_b", lay.linear2.bias),
                     ("norm_w", slice_fusion.norm.weight), ("norm_b", slice_fusion.norm.bias)):
        setattr(fw, field, hip.ptr(f32(t)))


def run_slice_fusion(fw: hip.FusionWeights, emb: torch.Tensor, B: int, D: int, mask: Optional[torch.Tensor], want_logits: bool,
                     want_probs: bool, ws_cache: dict):
    """mst_slice_fusion on slice embeddings [B*D, emb_in] -> (features [B, F], logits [B, out_ch] or None, the transformer's
    attention probabilities [B, heads, 1+D, 1+D] or None).  The mask ([B, D], nonzero = padding) and the probabilities exist for
    the transformer fusion only."""
    dev = emb.device
    transformer = fw.fusion_type == hip.FUSION_TRANSFORMER
    F = fw.emb * D if fw.fusion_type == hip.FUSION_LINEAR else fw.emb
    if want_logits and F != fw.head_in:                      # what nn.Linear raises in the reference (dino.py:166)
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({B}x{F} and {fw.head_in}x{fw.out_ch})")
    features = torch.empty((B, F), dtype=torch.float32, device=dev)
    logits = torch.empty((B, fw.out_ch), dtype=torch.float32, device=dev) if want_logits else None
    probs = torch.empty((B, fw.num_heads, D + 1, D + 1), dtype=torch.float32, device=dev) if want_probs and transformer else None
    m = None
    if mask is not None and transformer:
        m = mask.to(device=dev).to(torch.uint8).contiguous()
        if tuple(m.shape) != (B, D):
            raise RuntimeError(f"src_key_padding_mask must be [B, D] = {(B, D)}, got {tuple(m.shape)}")
    ws = cached_workspace(ws_cache, "fusion", hip.fusion_workspace_bytes(fw, B, D), dev)
    hip.slice_fusion(fw, emb.contiguous(), B, D, m, features, logits, probs, ws)
    return features, logits, probs
