"""The training mode of the HIP training steps (mst/train.py, mst/train_resnet.py): three model attributes, one validator, one resolver -- and
train_chunk_slices, the fourth attribute of DinoV2ClassifierSlice alone.

  train_precision 'fp32' (default) | 'bf16' | 'fp16' (env MST_TRAIN_PRECISION): MFMA operand type of the step's products -- the encoder
                  blocks' nn.Linear (forward, d input, d weight) of DinoV2ClassifierSlice, the convolutions and their two gradients of
                  ResNet / ResNetSliceTrans -- with fp32 accumulation; every other op stays fp32.  The reference trains under
                  Trainer(precision='16-mixed') (scripts/main_train.py:110-123).  'fp32' is exact fp32 MFMA, the mode the gradient parity
                  bar (1e-4 against float64 autograd, tests/test_train_gpu.py, tests/test_train_parity_gpu.py) is on.
  train_attention 'stored' (default) | 'flash' (env MST_TRAIN_ATTENTION; DinoV2ClassifierSlice only): 'stored' keeps the attention
                  probabilities of every block ([n, heads, N, N] fp32: 2.9 GB per block at 64 x 518^2).  'flash' (16-bit train_precision
                  only) is the reference's MemEffAttention: the encoder blocks keep the 16-bit q | k | v (written so by the QKV GEMM), the
                  output and the per-row log-sum-exp instead, and the backward recomputes the probabilities per tile
                  (csrc/k_attn16_train.hip: 16-bit flash forward, FlashAttention-2 backward with a separate deterministic dQ pass); no
                  [N, N] tensor exists.  The across-slice transformer's attention always stays on the stored path.
  train_storage   'fp32' (default) | '16bit' (env MST_TRAIN_STORAGE for DinoV2ClassifierSlice, MST_RESNET_TRAIN_STORAGE for the ResNets;
                  neither variable reaches the other family): what the step keeps for its backward lives in train_precision's 16-bit
                  type, as the reference's autocast keeps it.  It needs a 16-bit train_precision, and 'flash' where there is attention.
                  DinoV2: per token and block x0, x1 (the fp32 residual stream, what mst_layernorm_bwd reads; x0 of block i + 1 is x2 of
                  block i), xn1, xn2, a, br1, br2 [E] and qkv16 [3E], hpre, hact [4E] in 16 bits (SwiGLU blocks: x12 [2H] and h [H] in their place,
                  2H + H = 8E values as well) -- 40 E bytes plus the log-sum-exp instead of 66 E, and no 16-bit operand images beside them.  Each is written in 16 bits by its producer (the LayerNorm,
                  the GEMM epilogue, the attention epilogue, the GELU or mst_swiglu_fwd16) and is itself the operand of the forward product behind it, of that
                  product's weight gradient and of the elementwise backward kernels (csrc/k_train16.hip, k_train.hip, k_colsum.hip: residual + LayerScale + LayerNorm
                  in one pass, GELU 16 -> 16 and its derivative, the LayerScale gradient with a 16-bit factor, the transposed operand image
                  above 12,288 tokens; the flash kernels with a 16-bit output).
                  ResNet (csrc/k_bn.hip): z and y of every convolution + BatchNorm unit.  A unit takes its input in T, writes z in T
                  (mst_conv_gemm16) and y in T (mst_batchnorm_train16); that y IS the next unit's convolution operand, the operand of its
                  weight gradient and the residual of the unit that closes the block -- no fp32 activation, no second 16-bit copy, 4 bytes
                  per activation element instead of 10.  Backward: ONE mst_batchnorm_bwd16 per unit (ReLU mask, both sums, dz rounded to T,
                  the masked dy for the shortcut); its BatchNorm sums are fixed-order always.
                  Gradients stay fp32 in both (they are ~1e-6: csrc/k_attn16_train.hip), as do the residual stream, the weight-gradient
                  partials, the token stage, the slice transformer and the head.
  train_chunk_slices  0 (default) | k > 0 (env MST_TRAIN_CHUNK_SLICES; DinoV2ClassifierSlice only): recompute the encoder per chunk of k slices
                  instead of keeping its block state from forward to backward.  0 is the plain step.  With k > 0 the forward encodes the
                  flattened slice rows [B * D] (under slice sharding this rank's B * dl) k at a time and keeps only their embeddings; the
                  backward, behind the head and the slice transformer, runs per chunk the encoder forward again -- now saving -- and straight
                  into that chunk's backward, in the forward's chunk order.  The encoder has no statistic across slices (LayerNorm per token,
                  attention per slice), so this is the same function: the block state (66 E or 40 E bytes per token and block, above) is held
                  for k slices instead of all, at the price of one more encoder forward per step, issued chunk by chunk (on 's' the host's
                  issue time then bounds the step: take the largest k that fits).  A non-negative integer (`check_chunk`), never
                  inferred from the three attributes above and free to combine with each of their values; it may be changed between steps.
                  It is not the inference keyword chunk_slices / MST_CHUNK_SLICES.  ResNet and ResNetSliceTrans do not take it and the
                  variable does not reach them: their BatchNorm normalises with the statistics of the whole batch of slices, so a chunk's
                  forward is a different function from the batch's.

Every illegal combination is a ValueError from `check`, at construction (`from_kwargs`) and again at every call (`resolve`: the
attributes may have been changed since).

Autocast: a model whose train_precision was given neither by keyword nor by MST_TRAIN_PRECISION (the attribute then reads 'fp32' and
``_train_precision_given`` is False) takes the dtype of an enabled ``torch.autocast('cuda', dtype=torch.float16 | torch.bfloat16)`` region
around the forward, as the reference's Lightning trainer makes F.linear / F.conv2d do.  A given value -- an explicit 'fp32' included -- is
never overridden, nothing changes outside a region, the logits stay fp32, and train_attention / train_storage are never inferred.
`resolve` runs in the forward only; the resolved mode travels in the saved state, so the backward follows the forward's choice after the
region has ended.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple

import torch

_DTYPES = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}


class TrainMode(NamedTuple):
    mp: Optional[torch.dtype]                            # MFMA operand type of the step's products; None: exact fp32
    flash: bool                                          # train_attention == 'flash'
    storage16: bool                                      # train_storage == '16bit'
    chunk: int = 0                                       # train_chunk_slices: slices per recomputed encoder chunk; 0: the state is kept


def _dtype(precision: str) -> Optional[torch.dtype]:
    if precision not in _DTYPES:
        raise ValueError(f"train_precision must be 'fp32', 'bf16' or 'fp16' (got {precision!r})")
    return _DTYPES[precision]


def check(precision_is_16bit: bool, attention: str, storage: str, *, needs_flash: bool) -> Tuple[bool, bool]:
    """The one validator of the mode.  needs_flash: the model has attention blocks (DinoV2ClassifierSlice), so 16-bit storage also needs
    'flash'; a ResNet passes attention='stored' and False.  Returns (flash, storage16)."""
    if attention not in ("stored", "flash"):
        raise ValueError(f"train_attention must be 'stored' or 'flash' (got {attention!r})")
    if attention == "flash" and not precision_is_16bit:
        raise ValueError("train_attention='flash' needs train_precision 'bf16' or 'fp16' (the fp32 step is the exact-parity mode and keeps "
                         "the stored probabilities)")
    if storage not in ("fp32", "16bit"):
        raise ValueError(f"train_storage must be 'fp32' or '16bit' (got {storage!r})")
    if storage == "16bit" and not (precision_is_16bit and (attention == "flash" or not needs_flash)):
        raise ValueError("train_storage='16bit' needs train_precision 'bf16' or 'fp16'" + (" and train_attention='flash'" if needs_flash else "")
                         + " (the saved tensors are the 16-bit operands of the mixed-precision kernels)")
    return attention == "flash", storage == "16bit"


def check_chunk(value) -> int:
    """train_chunk_slices as a non-negative int.  Integers and their decimal strings (the environment's form) pass; a negative number, a
    fraction or anything else is a ValueError."""
    k = value
    if isinstance(k, str):
        try:
            k = int(k.strip())
        except ValueError:
            k = None
    elif isinstance(k, float) and k.is_integer():
        k = int(k)
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError(f"train_chunk_slices must be a non-negative integer: the slices per recomputed encoder chunk, 0 to keep the encoder's "
                         f"state (got {value!r})")
    return k


def chunk_from_kwargs(kwargs: dict) -> int:
    """DinoV2ClassifierSlice's constructor: pops train_chunk_slices from `kwargs`, defaulting to MST_TRAIN_CHUNK_SLICES and then 0."""
    return check_chunk(kwargs.pop("train_chunk_slices", os.environ.get("MST_TRAIN_CHUNK_SLICES", 0)))


def from_kwargs(kwargs: dict, *, storage_env: str, attention: bool) -> Tuple[str, str, str, bool]:
    """A model constructor's share: pops train_precision, train_attention (with `attention`: the model has attention blocks) and
    train_storage from `kwargs`, each defaulting to its environment variable (`storage_env`: the family's own), lower-cased and checked.
    Returns (train_precision, train_attention, train_storage, whether train_precision was given)."""
    given = "train_precision" in kwargs or "MST_TRAIN_PRECISION" in os.environ
    precision = str(kwargs.pop("train_precision", os.environ.get("MST_TRAIN_PRECISION", "fp32"))).lower()
    att = str(kwargs.pop("train_attention", os.environ.get("MST_TRAIN_ATTENTION", "stored"))).lower() if attention else "stored"
    storage = str(kwargs.pop("train_storage", os.environ.get(storage_env, "fp32"))).lower()
    check(_dtype(precision) is not None, att, storage, needs_flash=attention)
    return precision, att, storage, given


def resolve(model) -> TrainMode:
    """The mode of one training forward, from the model's attributes as they are now plus the autocast rule above."""
    precision = getattr(model, "train_precision", "fp32")
    mp = _dtype(precision)
    if precision == "fp32" and not getattr(model, "_train_precision_given", True) and torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        if dt in (torch.float16, torch.bfloat16):
            mp = dt
    flash, storage16 = check(mp is not None, getattr(model, "train_attention", "stored"), getattr(model, "train_storage", "fp32"),
                             needs_flash=hasattr(model, "train_attention"))
    # train_chunk_slices exists on DinoV2ClassifierSlice only: a ResNet resolves to 0 whatever the environment says
    return TrainMode(mp, flash, storage16, check_chunk(getattr(model, "train_chunk_slices", 0)))
