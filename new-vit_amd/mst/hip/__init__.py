"""ctypes binding of libmst_hip.so (C ABI: include/mst_hip.h).

PyTorch is used here only as plumbing: device memory (``tensor.data_ptr()``), the current HIP
stream and dtype tags.  There is NO fallback: if the library is missing or a call fails, a
``RuntimeError`` is raised (the product path never routes through torch ops or the CPU oracle).
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import Sequence, Optional, Tuple

import torch

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("MST_HIP_LIB", _HERE / "libmst_hip.so"))

F32, F16, BF16, F8E4M3 = 0, 1, 2, 3
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RELU, EPI_RESIDUAL, EPI_RESIDUAL_RELU, EPI_BIAS_SWIGLU = 0, 1, 2, 3, 4, 5
FFN_MLP, FFN_SWIGLU = 0, 1
FUSION_TRANSFORMER, FUSION_LINEAR, FUSION_AVERAGE = 0, 1, 2

_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}
TORCH_DT = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
DT_NAMES = {"fp32": F32, "f32": F32, "float32": F32, "fp16": F16, "f16": F16, "float16": F16,
            "bf16": BF16, "bfloat16": BF16,
            # e4m3 linear layers on a bf16 carrier (LayerNorm outputs, q/k/v, attention): mst_vit_weights.fp8_linear
            "fp8": BF16, "f8": BF16, "fp8_e4m3": BF16}
FP8_NAMES = ("fp8", "f8", "fp8_e4m3")

_vp, _i, _i64, _f, _d, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t


class VitLayer(C.Structure):
    _fields_ = [(n, _vp) for n in ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ls1",
                                   "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "ls2",
                                   "qkv_wf", "qkv_bf", "mlp_pack", "fc1_bf", "fc2_bf", "proj_pack", "proj_bf", "block_seq",
                                   "qkv_w8", "proj_w8", "fc1_w8", "fc2_w8")] + [("w8_scale", C.c_float * 4)]


class VitWeights(C.Structure):
    _fields_ = [("embed_dim", _i), ("depth", _i), ("num_heads", _i), ("num_registers", _i),
                ("compute_dtype", _i), ("grid_h", _i), ("grid_w", _i),
                ("patch_w", _vp), ("patch_b", _vp), ("prefix", _vp), ("pos_patch", _vp),
                ("layers", C.POINTER(VitLayer)), ("norm_w", _vp), ("norm_b", _vp), ("fp8_linear", _i),
                ("fp8_amax", _vp), ("fp8_amax_out", _vp), ("profiler", _vp), ("prune_last_block", _i),
                ("ffn_kind", _i), ("ffn_hidden", _i)]


class VitTaps(C.Structure):      # mst_vit_taps: blocks is a HOST array
    _fields_ = [("n_taps", _i), ("blocks", C.POINTER(_i)), ("norm", _i), ("out", _vp)]


class FusionWeights(C.Structure):
    _fields_ = [("emb_in", _i), ("emb", _i), ("out_ch", _i), ("fusion_type", _i), ("num_heads", _i)] + \
               [(n, _vp) for n in ("bottleneck_w", "bottleneck_b", "slice_pos_emb", "cls_token",
                                   "ln1_w", "ln1_b", "in_proj_w", "in_proj_b", "out_proj_w", "out_proj_b",
                                   "ln2_w", "ln2_b", "lin1_w", "lin1_b", "lin2_w", "lin2_b",
                                   "norm_w", "norm_b", "rope_freqs", "head_w", "head_b", "liere_rot")] + [("head_in", _i)]


# symbol -> (restype, argtypes); tests check every symbol of include/mst_hip.h is exported
SIGNATURES = {
    "mst_version": (_i, []),
    "mst_last_error": (C.c_char_p, []),
    "mst_layernorm": (_i, [_vp, _i64, _vp, _vp, _vp, _i, _i64, _i64, _i, _f, _vp]),
    "mst_gemm": (_i, [_vp, _i, _i64, _vp, _i64, _vp, _vp, _i, _i64, _i64, _i, _i, _i, _vp, _f, _i, _vp]),
    "mst_quantize_fp8": (_i, [_vp, _i, _i64, _vp, _vp, _vp]),
    "mst_gemm_fp8": (_i, [_vp, _i64, _vp, _i64, _vp, _vp, _f, _vp, _i, _i64, _i64, _i, _i, _i, _vp, _f, _i, _vp, _vp]),
    "mst_layernorm_fp8": (_i, [_vp, _i64, _vp, _vp, _vp, _i64, _i64, _i, _f, _vp, _vp]),
    "mst_attention": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "mst_attention_ex": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "mst_attention_cls": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "mst_gemm16_blocked": (_i, [_vp, _i, _vp, _i64, _vp, _vp, _i64, _i64, _i, _f, _i, _vp]),
    "mst_patch_rows16": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "mst_attention_cls_probs": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "mst_attention_probs_full": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "mst_attention_train_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mst_attention_train_fwd": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mst_attention_train_bwd": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "mst_attention_train_fwd16": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mst_attention_train_bwd16": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _sz, _vp]),
    "mst_pos_embed_interp": (_i, [_vp, _i, _i, _i, _i, _d, _i, _vp, _vp]),
    "mst_mlp_fused": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i64, _i, _f, _vp]),
    "mst_block_fused_scratch_bytes": (_sz, []),
    "mst_block_fused": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i64, _i, _f, _vp]),
    "mst_block_fused_s": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i64, _i, _f, _i, _vp]),
    "mst_gemm_ex": (_i, [_vp, _vp, _vp, _i, _i, _i, C.POINTER(_i64), _i, _i, _f, _f, _vp]),
    "mst_softmax_rows": (_i, [_vp, _vp, _i64, _i, _i, _vp]),
    "mst_softmax_rows_bwd": (_i, [_vp, _vp, _i64, _i, _f, _vp]),
    "mst_layernorm_bwd": (_i, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i, _f, _vp]),
    "mst_act_fwd": (_i, [_vp, _vp, _i64, _i, _vp]),
    "mst_act_bwd": (_i, [_vp, _vp, _i64, _i, _vp]),
    "mst_swiglu_fwd": (_i, [_vp, _vp, _i64, _i, _vp]),
    "mst_swiglu_bwd": (_i, [_vp, _vp, _vp, _i64, _i, _vp]),
    "mst_colsum": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp, _vp]),
    "mst_axpby_cols": (_i, [_vp, _i64, _vp, _f, _f, _vp, _i64, _i64, _i, _vp]),
    "mst_im2col14": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "mst_pos_embed_interp_bwd": (_i, [_vp, _i, _i, _i, _i, _d, _vp, _vp]),
    "mst_patch_embed_dgrad": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    # the three-channel patch embedding at the op level: forward, input gradient, split weight gradient (csrc/k_features.hip, k_patch_dgrad.hip)
    "mst_patch_embed_rgb": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "mst_patch_embed_rgb_dgrad": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _vp]),
    "mst_patch_embed_rgb_wgrad": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp, _vp]),
    # 16-bit storage mode of the training step (csrc/k_train16.hip; act / swiglu in k_train.hip, the column sums in k_colsum.hip)
    "mst_residual_layernorm16": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64, _i, _f, _vp]),
    "mst_act_fwd16": (_i, [_vp, _vp, _i, _i64, _i, _vp]),
    "mst_act_bwd16": (_i, [_vp, _i, _vp, _i64, _i, _vp]),
    "mst_swiglu_fwd16": (_i, [_vp, _vp, _i, _i64, _i, _vp]),
    "mst_swiglu_bwd16": (_i, [_vp, _i, _vp, _vp, _i64, _i, _vp]),
    "mst_colsum_b16": (_i, [_vp, _i64, _vp, _i, _i64, _i64, _i, _vp, _vp]),
    "mst_colsum_b16_ordered": (_i, [_vp, _i64, _vp, _i, _i64, _i64, _i, _vp, _vp, _sz, _vp]),
    "mst_transpose16": (_i, [_vp, _i, _i64, _i64, _i, _vp, _i64, _i64, _vp]),
    # 16-bit storage mode of the ResNet training step (csrc/k_bn.hip)
    "mst_batchnorm_train16_workspace_bytes": (_sz, [_i64, _i]),
    "mst_batchnorm_train16": (_i, [_vp, _i, _i64, _i, _vp, _vp, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mst_batchnorm_bwd16_workspace_bytes": (_sz, [_i64, _i]),
    "mst_batchnorm_bwd16": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mst_maxpool_bwd_nhwc16_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mst_maxpool_bwd_nhwc16": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mst_avgpool_nhwc16": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "mst_im2col_nhwc": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "mst_cvt16": (_i, [_vp, _i64, _i64, _i, _f, _vp, _i, _i64, _i, _i64, _vp]),
    "mst_gemm16_splitk": (_i, [_vp, _i, _i64, _vp, _i64, _vp, _i64, _i64, _i, _i, _i, _i64, _vp]),
    "mst_conv_gemm": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "mst_conv_gemm16": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "mst_rope_rows": (_i, [_vp, _i64, _i, _i, _i, _vp, _f, _vp]),
    "mst_cvt32": (_i, [_vp, _i, _i64, _vp, _vp]),
    "mst_im2col_nhwc16": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp]),
    "mst_maxpool_nhwc16": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "mst_conv_wgrad": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i64, _vp]),
    "mst_conv_wgrad16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i64, _vp]),
    "mst_conv_dgrad": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp]),
    "mst_conv_dgrad_stem": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _i, _vp, _vp]),
    "mst_maxpool_nhwc": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "mst_avgpool_nhwc": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mst_batchnorm_train": (_i, [_vp, _i64, _i, _vp, _vp, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "mst_batchnorm_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _vp, _vp, _vp, _vp]),
    "mst_col2im_nhwc": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "mst_maxpool_bwd_nhwc": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "mst_avgpool_bwd_nhwc": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mst_gradcampp": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "mst_crop_or_pad": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "mst_znorm_state_bytes": (_sz, []),
    "mst_znorm": (_i, [_vp, _i64, _f, _f, _vp, _vp, _vp]),
    "mst_crop_or_pad_at": (_i, [_vp, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp, _sz, _vp]),
    "mst_augment_volumes": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _vp, C.c_uint64, C.c_uint64, _vp]),
    "mst_volume_min": (_i, [_vp, _i, _i, _i64, _vp, _i, _vp]),
    "mst_slices2rgb": (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    "mst_patch_embed": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp]),
    "mst_vit_workspace_bytes": (_sz, [C.POINTER(VitWeights), _i, _i, _i]),
    "mst_vit_encode": (_i, [C.POINTER(VitWeights), _vp, _i, _i, _i, _i, _vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "mst_vit_features_workspace_bytes": (_sz, [C.POINTER(VitWeights), _i, _i, _i, _i]),
    "mst_vit_encode_features": (_i, [C.POINTER(VitWeights), _vp, _i, _i, _i, _i, _i, _vp, _vp, C.POINTER(VitTaps), _i, _vp, _sz, _vp]),
    "mst_fusion_workspace_bytes": (_sz, [C.POINTER(FusionWeights), _i, _i]),
    "mst_slice_fusion": (_i, [C.POINTER(FusionWeights), _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mst_attention_readout": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "mst_saliency_accumulate": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mst_saliency_upsample": (_i, [_vp, _i, _i, _i, _f, _i, _i, _i, _vp, _vp]),
    # folded test-time augmentation (csrc/k_tta.hip)
    "mst_tta_inplane_flips": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "mst_saliency_accumulate_tta": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mst_liere_rotation": (_i, [_vp, _i, _i, _i, _vp, _vp]),
    "mst_attention_rollout": (_i, [C.POINTER(_vp), _i, _i64, _i, _vp, _vp, _vp]),
    # fixed-order forms (torch.use_deterministic_algorithms): no floating-point atomics, caller-given workspace
    "mst_colsum_ordered_workspace_bytes": (_sz, [_i64, _i]),
    "mst_colsum_ordered": (_i, [_vp, _i64, _vp, _i64, _i64, _i, _vp, _vp, _sz, _vp]),
    "mst_layernorm_bwd_ordered_workspace_bytes": (_sz, [_i64, _i]),
    "mst_layernorm_bwd_ordered": (_i, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i, _f, _vp, _sz, _vp]),
    "mst_batchnorm_train_ordered_workspace_bytes": (_sz, [_i64, _i]),
    "mst_batchnorm_train_ordered": (_i, [_vp, _i64, _i, _vp, _vp, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mst_batchnorm_bwd_ordered_workspace_bytes": (_sz, [_i64, _i]),
    "mst_batchnorm_bwd_ordered": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "mst_col2im_nhwc_gather": (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "mst_maxpool_bwd_nhwc_gather_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mst_maxpool_bwd_nhwc_gather": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "mst_pos_embed_interp_bwd_ordered_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "mst_pos_embed_interp_bwd_ordered": (_i, [_vp, _i, _i, _i, _i, _d, _vp, _vp, _sz, _vp]),
    "mst_znorm_ordered_workspace_bytes": (_sz, [_i64]),
    "mst_znorm_ordered": (_i, [_vp, _i64, _f, _f, _vp, _vp, _vp, _sz, _vp]),
    "mst_profiler_create": (_vp, []),
    "mst_profiler_destroy": (None, [_vp]),
    "mst_profiler_collect": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "mst_kernel_kind_name": (C.c_char_p, [_i]),
}
K_COUNT = 10
ABI_VERSION = 300        # mst_version(): round 3 (mst_vit_layer.block_seq, mst_block_fused_s)

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """dlopen the library once; raises RuntimeError (never falls back) when it is absent."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"libmst_hip.so not found at {LIB_PATH}: build it with `python new-vit_amd/build.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU / PyTorch fallback for the MST hot path.")
        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.mst_version() != ABI_VERSION:             # the struct mirrors below follow include/mst_hip.h of exactly this version
            raise RuntimeError(f"{LIB_PATH} reports ABI version {lib.mst_version()}, this binding was written for {ABI_VERSION}: "
                               "rebuild with `python new-vit_amd/build.py --force`")
        _lib = lib
    return _lib


def last_error() -> str:
    return (load().mst_last_error() or b"").decode()


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed (status {rc}): {last_error()}")


def dt_of(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"unsupported dtype {t.dtype}") from None


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def stream_of(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def deterministic() -> bool:
    """torch.use_deterministic_algorithms(True) (warn_only or not) is in force: every floating-point reduction of the training steps and
    of preprocess.znormalize then takes its fixed-order entry point (mst_*_ordered / *_gather), bit-reproducible for fixed shapes.  Read
    at every call, so that toggling the flag between steps takes effect."""
    return torch.are_deterministic_algorithms_enabled()


def workspace(nbytes: int, device) -> Optional[torch.Tensor]:
    """Device scratch of `nbytes` bytes for an entry point's `workspace` argument (None for 0: the library accepts NULL then)."""
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device) if nbytes else None


def _call_ws(name: str, size_args, t: torch.Tensor, *args, sized_by: Optional[str] = None):
    """Call entry point `name`, whose last three arguments are (workspace, workspace_bytes, stream), with `args` in front of them: the size
    is `<sized_by or name>_workspace_bytes(*size_args)`, the scratch comes from workspace() on t's device (NULL / 0 for 0 bytes), the
    stream is t's current one."""
    lib = load()
    ws = workspace(getattr(lib, (sized_by or name) + "_workspace_bytes")(*size_args), t.device)
    _check(getattr(lib, name)(*args, ptr(ws), 0 if ws is None else ws.numel(), stream_of(t)), name)


def _dev(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor must live on a HIP device (got {t.device}); the MST kernels have no CPU path")
    if not t.is_contiguous():
        raise RuntimeError(f"{what}: tensor must be contiguous")


# ---- per-op wrappers (unit parity tests call these; the models call the orchestrators) --------
def layernorm(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
              out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    _dev(x, "layernorm")
    rows, cols = x.numel() // x.shape[-1], x.shape[-1]
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    _check(load().mst_layernorm(ptr(x), cols, ptr(weight), ptr(bias), ptr(out), _DT[out_dtype], cols, rows, cols,
                                eps, stream_of(x)), "mst_layernorm")
    return out


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], *, epilogue: int = EPI_BIAS,
         out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None,
         gamma: Optional[torch.Tensor] = None, col_scale: float = 1.0, scale_cols: int = 0) -> torch.Tensor:
    _dev(a, "gemm")
    _dev(w, "gemm")
    M, K = a.shape
    N = w.shape[0]
    n_out = N // 2 if epilogue == EPI_BIAS_SWIGLU else N     # w is the row-paired w12 image (pack_swiglu): gate and value rows give one column
    if out is None:
        out = torch.empty((M, n_out), dtype=out_dtype or a.dtype, device=a.device)
    _check(load().mst_gemm(ptr(a), dt_of(a), K, ptr(w), K, ptr(bias), ptr(out), dt_of(out), n_out, M, N, K, epilogue,
                           ptr(gamma), col_scale, scale_cols, stream_of(a)), "mst_gemm")
    return out


F8_MAX = 448.0      # largest finite OCP e4m3


def quantize_weight_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, float]:
    """Per-tensor e4m3 form of a weight matrix: (bytes [out,in] uint8, scale = max|W|/448), W ~ scale * e4m3(bytes).  Done
    once per weight version with torch's round-to-nearest-even cast (host-side preparation, like the other packers)."""
    w = w.detach().to(torch.float32)
    amax = float(w.abs().max())
    scale = amax / F8_MAX if amax > 0 else 1.0
    q = (w / scale).clamp(-F8_MAX, F8_MAX).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale


def quantize_fp8(x: torch.Tensor, amax: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """mst_quantize_fp8: (e4m3 bytes with x's shape, amax fp32 [1] on the device)."""
    _dev(x, "quantize_fp8")
    if amax is None:
        amax = torch.zeros(1, dtype=torch.float32, device=x.device)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _check(load().mst_quantize_fp8(ptr(x), dt_of(x), x.numel(), ptr(amax), ptr(out), stream_of(x)), "mst_quantize_fp8")
    return out, amax


def gemm_fp8(a8: torch.Tensor, a_amax: torch.Tensor, w8: torch.Tensor, w_scale: float, bias: Optional[torch.Tensor], *,
             epilogue: int = EPI_BIAS, out: Optional[torch.Tensor] = None, out_dtype: torch.dtype = torch.float32,
             gamma: Optional[torch.Tensor] = None, col_scale: float = 1.0, scale_cols: int = 0,
             c_amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """c_amax given: the output is e4m3 bytes (uint8) under that calibrated scale."""
    _dev(a8, "gemm_fp8")
    _dev(w8, "gemm_fp8")
    M, K = a8.shape
    N = w8.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.uint8 if c_amax is not None else out_dtype, device=a8.device)
    cdt = F8E4M3 if c_amax is not None else dt_of(out)
    _check(load().mst_gemm_fp8(ptr(a8), K, ptr(w8), K, ptr(bias), ptr(a_amax), w_scale, ptr(out), cdt, N, M, N, K,
                               epilogue, ptr(gamma), col_scale, scale_cols, ptr(c_amax), stream_of(a8)), "mst_gemm_fp8")
    return out


def layernorm_fp8(x: torch.Tensor, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float,
                  amax: torch.Tensor) -> torch.Tensor:
    """mst_layernorm_fp8: LayerNorm over the last dim of fp32 x [rows, cols] -> e4m3 bytes under the calibrated scale."""
    _dev(x, "layernorm_fp8")
    rows, cols = x.shape
    out = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    _check(load().mst_layernorm_fp8(ptr(x), cols, ptr(gamma), ptr(beta), ptr(out), cols, rows, cols, eps, ptr(amax),
                                    stream_of(x)), "mst_layernorm_fp8")
    return out


ATTN_LOG2Q, ATTN_OUT_BLOCKED = 1, 2      # mst_attention_flags


def _operand(t, what: str, name: str, dtypes, shape=None):
    """A tensor of one of `dtypes` and, where given, of `shape`: the first half of what every wrapper of the encoder's seam kernels checks
    before the library is reached (_resident is the second: types and shapes are refused first, wherever the tensors live)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor")
    if t.dtype not in dtypes:
        raise TypeError(f"{what}: {name} is {t.dtype} ({', '.join(str(d).replace('torch.', '') for d in dtypes)})")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {list(shape)}, got {list(t.shape)}")


def _resident(what: str, **tensors):
    """Every tensor (None skipped) contiguous and on one HIP device."""
    first = None
    for name, t in tensors.items():
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError(f"{what}: {name} must live on a HIP device (got {t.device}); the MST kernels have no CPU path")
        first = t if first is None else first
        if t.device != first.device:
            raise ValueError(f"{what}: {name} is on {t.device}, not on {first.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be contiguous")


def storage_rows(t: torch.Tensor, cols: int) -> int:
    """Whole rows of `cols` elements that t's storage holds from t's first element on (a `buf[:M]` view of a padded buffer counts the
    padding: what a kernel may touch behind the view is the allocation's, not the view's)."""
    return (t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()) // cols


def _whole_groups(what: str, M: int, cols: int, **tensors):
    """Operands in the blocked / image layouts (include/mst_hip.h, mst_layout_flags) are read and written as whole 32-row groups: every
    tensor given (None skipped) must be backed by ceil(M / 32) * 32 rows of storage, or the call is refused before any launch."""
    need = (M + 31) // 32 * 32
    for name, t in tensors.items():
        if t is not None and storage_rows(t, cols) < need:
            raise ValueError(f"{what}: {name} is backed by {storage_rows(t, cols)} rows of storage, the blocked / image layouts take "
                             f"whole 32-row groups: {need} rows for M = {M}")


_T16 = (torch.bfloat16, torch.float16)


def attention(qkv: torch.Tensor, n_seq: int, N: int, heads: int, head_dim: int = 64, *, log2q: bool = False, out_blocked: bool = False,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mst_attention.  log2q / out_blocked / out given: mst_attention_ex, the 16-bit kernel as mst_vit_encode launches it -- log2q: q is
    pre-multiplied by head_dim^-0.5 * log2 e; out_blocked: the result comes back in the 16-bit blocked layout, [ceil(n_seq*N / 32) * 32,
    heads*64] (decode with from_blocked16; rows past n_seq*N are not written).  out: the buffer to write, at least that many rows (more
    are allowed: tests put guard rows behind it); it is returned as given."""
    if not (log2q or out_blocked or out is not None):
        _dev(qkv, "attention")
        out = torch.empty((n_seq * N, heads * head_dim), dtype=qkv.dtype, device=qkv.device)
        _check(load().mst_attention(ptr(qkv), dt_of(qkv), n_seq, N, heads, head_dim, ptr(out), stream_of(qkv)), "mst_attention")
        return out
    if min(n_seq, N, heads) < 1 or head_dim != 64:
        raise ValueError(f"attention: n_seq={n_seq} N={N} heads={heads} head_dim={head_dim} (positive sizes, head_dim 64)")
    _operand(qkv, "attention", "qkv", _T16, (n_seq * N, 3 * heads * 64))
    rows = (n_seq * N + 31) // 32 * 32 if out_blocked else n_seq * N
    if out is not None:
        _operand(out, "attention", "out", (qkv.dtype,))
        if out.dim() != 2 or out.shape[1] != heads * 64 or out.shape[0] < rows:
            raise ValueError(f"attention: out must be [>= {rows}, {heads * 64}], got {list(out.shape)}")
    _resident("attention", qkv=qkv, out=out)
    if out is None:
        out = torch.empty((rows, heads * 64), dtype=qkv.dtype, device=qkv.device)
    flags = (ATTN_LOG2Q if log2q else 0) | (ATTN_OUT_BLOCKED if out_blocked else 0)
    _check(load().mst_attention_ex(ptr(qkv), dt_of(qkv), n_seq, N, heads, 64, ptr(out), flags, stream_of(qkv)), "mst_attention_ex")
    return out


def attention_cls(qkv: torch.Tensor, n_seq: int, N: int, heads: int, *, log2q: bool = False, probs: bool = True):
    """mst_attention_cls: (out [n_seq, heads*64] in qkv's type, probs fp32 [n_seq, heads, N] or None) of the CLS query (row 0 of every
    sequence); qkv fp32 / fp16 / bf16, head_dim 64."""
    if min(n_seq, N, heads) < 1:
        raise ValueError(f"attention_cls: n_seq={n_seq} N={N} heads={heads}")
    _operand(qkv, "attention_cls", "qkv", (torch.float32,) + _T16, (n_seq * N, 3 * heads * 64))
    _resident("attention_cls", qkv=qkv)
    out = torch.empty((n_seq, heads * 64), dtype=qkv.dtype, device=qkv.device)
    pr = torch.empty((n_seq, heads, N), dtype=torch.float32, device=qkv.device) if probs else None
    _check(load().mst_attention_cls(ptr(qkv), dt_of(qkv), n_seq, N, heads, ptr(out), ptr(pr), 1 if log2q else 0, stream_of(qkv)),
           "mst_attention_cls")
    return out, pr


def gemm_blocked(a_blocked: torch.Tensor, M: int, w: torch.Tensor, bias: Optional[torch.Tensor], *, col_scale: float = 1.0,
                 scale_cols: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mst_gemm16_blocked: the first M rows of a_blocked (16-bit blocked layout, [>= ceil(M / 32) * 32, 384]) times w [N, 384]^T + bias,
    columns below scale_cols times col_scale -> row-major [M, N] in the operand type.  Raises where the weights-in-registers kernel
    does not take the shape (there is no other kernel that reads blocked rows)."""
    _operand(a_blocked, "gemm_blocked", "a_blocked", _T16)
    if a_blocked.dim() != 2 or a_blocked.shape[1] != 384 or a_blocked.shape[0] % 32 or not 0 < M <= a_blocked.shape[0]:
        raise ValueError(f"gemm_blocked: a_blocked must be whole 32-row groups [>= M, 384] with M = {M} > 0, got {list(a_blocked.shape)}")
    _operand(w, "gemm_blocked", "w", (a_blocked.dtype,))
    if w.dim() != 2 or w.shape[1] != 384:
        raise ValueError(f"gemm_blocked: w must be [N, 384], got {list(w.shape)}")
    N = w.shape[0]
    if bias is not None:
        _operand(bias, "gemm_blocked", "bias", (torch.float32,), (N,))
    if out is not None:
        _operand(out, "gemm_blocked", "out", (a_blocked.dtype,), (M, N))
    _resident("gemm_blocked", a_blocked=a_blocked, w=w, bias=bias, out=out)
    if out is None:
        out = torch.empty((M, N), dtype=a_blocked.dtype, device=a_blocked.device)
    _check(load().mst_gemm16_blocked(ptr(a_blocked), dt_of(a_blocked), ptr(w), 384, ptr(bias), ptr(out), N, M, N, col_scale, scale_cols,
                                     stream_of(a_blocked)), "mst_gemm16_blocked")
    return out


def patch_rows16(vol: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, prefix: torch.Tensor, pos_patch: torch.Tensor):
    """mst_patch_rows16: patch_embed for E = 384 that also writes the plain LayerNorm of every row -> (x fp32 [n, N, 384], xn [n, N, 384]
    in wp's 16-bit type).  vol [n, H, W] fp32 / fp16 / bf16, wp [384, 224] bf16 / fp16, bias [384], prefix [1+R, 384], pos_patch [Np, 384]."""
    _operand(vol, "patch_rows16", "vol", (torch.float32,) + _T16)
    if vol.dim() != 3 or vol.shape[1] % 14 or vol.shape[2] % 14 or 0 in vol.shape:
        raise ValueError(f"patch_rows16: vol must be [n, H, W] with H and W multiples of 14, got {list(vol.shape)}")
    n, H, W = vol.shape
    Np = (H // 14) * (W // 14)
    _operand(wp, "patch_rows16", "wp", _T16, (384, 224))
    _operand(bias, "patch_rows16", "bias", (torch.float32,), (384,))
    _operand(prefix, "patch_rows16", "prefix", (torch.float32,))
    if prefix.dim() != 2 or prefix.shape[0] < 1 or prefix.shape[1] != 384:
        raise ValueError(f"patch_rows16: prefix must be [1+R, 384], got {list(prefix.shape)}")
    _operand(pos_patch, "patch_rows16", "pos_patch", (torch.float32,), (Np, 384))
    _resident("patch_rows16", vol=vol, wp=wp, bias=bias, prefix=prefix, pos_patch=pos_patch)
    n_prefix = prefix.shape[0]
    x = torch.empty((n, n_prefix + Np, 384), dtype=torch.float32, device=vol.device)
    xn = torch.empty((n, n_prefix + Np, 384), dtype=wp.dtype, device=vol.device)
    _check(load().mst_patch_rows16(ptr(vol), dt_of(vol), n, H, W, ptr(wp), dt_of(wp), ptr(bias), ptr(prefix), n_prefix, ptr(pos_patch),
                                   ptr(x), ptr(xn), stream_of(vol)), "mst_patch_rows16")
    return x, xn


def attention_cls_probs(qkv: torch.Tensor, n_seq: int, N: int, heads: int, head_dim: int = 64) -> torch.Tensor:
    _dev(qkv, "attention_cls_probs")
    out = torch.empty((n_seq, heads, N), dtype=torch.float32, device=qkv.device)
    _check(load().mst_attention_cls_probs(ptr(qkv), dt_of(qkv), n_seq, N, heads, head_dim, ptr(out), stream_of(qkv)),
           "mst_attention_cls_probs")
    return out


def attention_probs_full(qkv: torch.Tensor, n_seq: int, N: int, heads: int, head_dim: int = 64) -> torch.Tensor:
    _dev(qkv, "attention_probs_full")
    out = torch.empty((n_seq, heads, N, N), dtype=torch.float32, device=qkv.device)
    _check(load().mst_attention_probs_full(ptr(qkv), dt_of(qkv), n_seq, N, heads, head_dim, ptr(out), stream_of(qkv)),
           "mst_attention_probs_full")
    return out


def _train_attn_args(qkv16: torch.Tensor, n_seq: int, N: int, heads: int, head_dim: int, what: str):
    _dev(qkv16, what)
    if qkv16.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{what}: qkv16 must be bf16 or fp16 (got {qkv16.dtype})")
    if n_seq < 1 or N < 1 or heads < 1 or tuple(qkv16.shape) != (n_seq * N, 3 * heads * head_dim):
        raise ValueError(f"{what}: qkv16 {tuple(qkv16.shape)} is not [n_seq*N, 3*heads*head_dim] for n_seq={n_seq} N={N} heads={heads} "
                         f"head_dim={head_dim}")


def _f32_like(t: torch.Tensor, shape, dev, what: str, name: str):
    _dev(t, what)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != dev:
        raise ValueError(f"{what}: {name} must be fp32 {tuple(shape)} on {dev} (got {t.dtype} {tuple(t.shape)} on {t.device})")


def attention_train_fwd(qkv16: torch.Tensor, n_seq: int, N: int, heads: int, head_dim: int = 64,
                        out_dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """mst_attention_train_fwd: (out fp32 [n_seq*N, heads*head_dim], lse fp32 [n_seq, heads, N], natural log) of the training step's
    memory-efficient attention on 16-bit packed q | k | v rows (q pre-scaled).  out_dtype = qkv16's own type: mst_attention_train_fwd16,
    the same output rounded to that type by the kernel's epilogue."""
    _train_attn_args(qkv16, n_seq, N, heads, head_dim, "attention_train_fwd")
    if out_dtype not in (torch.float32, qkv16.dtype):
        raise ValueError(f"attention_train_fwd: out_dtype must be fp32 or qkv16's {qkv16.dtype} (got {out_dtype})")
    out = torch.empty((n_seq * N, heads * head_dim), dtype=out_dtype, device=qkv16.device)
    lse = torch.empty((n_seq, heads, N), dtype=torch.float32, device=qkv16.device)
    lib = load()
    fn, what = (lib.mst_attention_train_fwd, "mst_attention_train_fwd") if out_dtype == torch.float32 else \
               (lib.mst_attention_train_fwd16, "mst_attention_train_fwd16")
    _check(fn(ptr(qkv16), dt_of(qkv16), n_seq, N, heads, head_dim, ptr(out), ptr(lse), stream_of(qkv16)), what)
    return out, lse


def attention_train_bwd(qkv16: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse: torch.Tensor, n_seq: int, N: int, heads: int,
                        dq_scale: float = 1.0, head_dim: int = 64, dqkv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mst_attention_train_bwd: the gradient of the packed rows, dqkv fp32 [n_seq*N, 3*heads*head_dim] (dQ times dq_scale), from the
    forward's qkv16 / out / lse and dout = d out.  Every element of dqkv is written; no [N, N] tensor is allocated.  `out` is fp32, or in
    qkv16's own type as attention_train_fwd(out_dtype=...) wrote it (mst_attention_train_bwd16)."""
    what = "attention_train_bwd"
    _train_attn_args(qkv16, n_seq, N, heads, head_dim, what)
    dev = qkv16.device
    out16 = out.dtype == qkv16.dtype
    if out16:
        _dev(out, what)
        if tuple(out.shape) != (n_seq * N, heads * head_dim) or out.device != dev:
            raise ValueError(f"{what}: out must be [{n_seq * N}, {heads * head_dim}] on {dev} (got {tuple(out.shape)} on {out.device})")
    else:
        _f32_like(out, (n_seq * N, heads * head_dim), dev, what, "out")
    _f32_like(dout, (n_seq * N, heads * head_dim), dev, what, "dout")
    _f32_like(lse, (n_seq, heads, N), dev, what, "lse")
    if dqkv is None:
        dqkv = torch.empty((n_seq * N, 3 * heads * head_dim), dtype=torch.float32, device=dev)
    _f32_like(dqkv, (n_seq * N, 3 * heads * head_dim), dev, what, "dqkv")
    # (0 bytes only for sizes the library refuses before it looks at the workspace: no minimum needed)
    _call_ws("mst_attention_train_bwd16" if out16 else "mst_attention_train_bwd", (n_seq, N, heads, head_dim), qkv16,
             ptr(qkv16), dt_of(qkv16), ptr(out), ptr(dout), ptr(lse), n_seq, N, heads, head_dim, dq_scale, ptr(dqkv),
             sized_by="mst_attention_train_bwd")
    return dqkv


def pos_embed_interp(pos_patch: torch.Tensor, M: int, gh: int, gw: int, offset: float = 0.1,
                     antialias: bool = False) -> torch.Tensor:
    _dev(pos_patch, "pos_embed_interp")
    E = pos_patch.shape[-1]
    out = torch.empty((gh * gw, E), dtype=torch.float32, device=pos_patch.device)
    _check(load().mst_pos_embed_interp(ptr(pos_patch), M, E, gh, gw, offset, 1 if antialias else 0, ptr(out), stream_of(pos_patch)),
           "mst_pos_embed_interp")
    return out


def patch_embed(vol: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, prefix: torch.Tensor,
                pos_patch: torch.Tensor) -> torch.Tensor:
    _dev(vol, "patch_embed")
    n, H, W = vol.shape
    E = wp.shape[0]
    n_prefix = prefix.shape[0]
    N = n_prefix + (H // 14) * (W // 14)
    x = torch.empty((n, N, E), dtype=torch.float32, device=vol.device)
    _check(load().mst_patch_embed(ptr(vol), dt_of(vol), n, H, W, ptr(wp), dt_of(wp), ptr(bias), ptr(prefix), n_prefix,
                                  ptr(pos_patch), E, ptr(x), stream_of(vol)), "mst_patch_embed")
    return x


def slices2rgb(vol: torch.Tensor) -> torch.Tensor:
    """mst_slices2rgb: [B,1,D,H,W] -> [B*ceil(D/3), 3, H, W] (reference dino.py:10-27)."""
    _dev(vol, "slices2rgb")
    B, C, D, H, W = vol.shape
    assert C == 1, "More than one channel"              # dino.py:14
    Dp = (D + 2) // 3 * 3
    out = torch.empty((B * Dp // 3, 3, H, W), dtype=vol.dtype, device=vol.device)
    _check(load().mst_slices2rgb(ptr(vol), dt_of(vol), B, D, H, W, ptr(out), stream_of(vol)), "mst_slices2rgb")
    return out


AUG_COS, AUG_SIN, AUG_FILL, AUG_SIGN, AUG_STD, AUG_FLIP_D, AUG_FLIP_H, AUG_FLIP_W, AUG_REC = 0, 1, 2, 3, 4, 5, 6, 7, 8    # record of mst_augment_volumes


def volume_min(x: torch.Tensor, out: Optional[torch.Tensor] = None, column: int = 0) -> torch.Tensor:
    """mst_volume_min: the minimum of every volume of x [n, ...] (fp32 / fp16 / bf16) as fp32 [n]; or, out fp32 [n, K] given, written into
    out[:, column] (the fill of mst_augment_volumes' records) and out returned."""
    _operand(x, "volume_min", "x", (torch.float32,) + _T16)
    if x.dim() < 2 or 0 in x.shape:
        raise ValueError(f"volume_min: x must be [n, ...] and not empty, got {list(x.shape)}")
    n = x.shape[0]
    if out is not None:
        _operand(out, "volume_min", "out", (torch.float32,))
        if out.dim() != 2 or out.shape[0] != n or not 0 <= column < out.shape[1]:
            raise ValueError(f"volume_min: out must be [{n}, > {column}], got {list(out.shape)}")
    _resident("volume_min", x=x, out=out)
    res = out if out is not None else torch.empty((n, 1), dtype=torch.float32, device=x.device)
    _check(load().mst_volume_min(ptr(x), dt_of(x), n, x.numel() // n, res.data_ptr() + 4 * column, res.shape[1], stream_of(x)), "mst_volume_min")
    return out if out is not None else res[:, 0]


def augment_volumes(x: torch.Tensor, params: torch.Tensor, seed: int = 0, counter: int = 0,
                    out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """mst_augment_volumes: x [n, D, H, W] (fp32 / fp16 / bf16) rotated in plane, flipped, sign-inverted and noised per its record
    params [n, 8] fp32 (cos, sin, fill, sign, noise_std, flipD, flipH, flipW; include/mst_hip.h) -> a new tensor of out_dtype (x's own
    by default).  seed / counter: the 64-bit Philox key and the counter of volume 0 (volume v uses counter + v)."""
    _operand(x, "augment_volumes", "x", (torch.float32,) + _T16)
    if x.dim() != 4 or 0 in x.shape:
        raise ValueError(f"augment_volumes: x must be [n, D, H, W] and not empty, got {list(x.shape)}")
    n, D, H, W = x.shape
    _operand(params, "augment_volumes", "params", (torch.float32,), (n, AUG_REC))
    out_dtype = out_dtype or x.dtype
    if out_dtype not in _DT:
        raise TypeError(f"augment_volumes: out_dtype {out_dtype} (float32, float16, bfloat16)")
    _resident("augment_volumes", x=x, params=params)
    out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mask = (1 << 64) - 1
    _check(load().mst_augment_volumes(ptr(x), dt_of(x), ptr(out), _DT[out_dtype], n, D, H, W, ptr(params), int(seed) & mask, int(counter) & mask,
                                      stream_of(x)), "mst_augment_volumes")
    return out


def mlp_fused(x: torch.Tensor, wpack: torch.Tensor, b1f: torch.Tensor, b2f: torch.Tensor,
              xn_out: Optional[torch.Tensor], dtype: torch.dtype, eps: float = 1e-6):
    """x [M,384] fp32 updated in place; xn_out (optional, `dtype`) receives normalise(x_new).
    wpack / b1f / b2f from pack_mlp (LayerNorm affine and LayerScale folded)."""
    _dev(x, "mlp_fused")
    M, E = x.shape
    _check(load().mst_mlp_fused(ptr(x), ptr(xn_out), _DT[dtype], ptr(wpack), ptr(b1f), ptr(b2f), M, E, eps,
                                stream_of(x)), "mst_mlp_fused")


def block_fused(x: torch.Tensor, attn_out: torch.Tensor, proj_pack: torch.Tensor, proj_bf: torch.Tensor, wpack: torch.Tensor,
                b1f: torch.Tensor, b2f: torch.Tensor, xn_out: Optional[torch.Tensor], eps: float = 1e-6,
                scratch: Optional[torch.Tensor] = None):
    """mst_block_fused: x [M,384] fp32 in place += ls1*proj(attn_out) then += the fused MLP; xn_out (may be attn_out itself)
    receives normalise(x_new).  proj_pack / proj_bf from pack_proj, wpack / b1f / b2f from pack_mlp."""
    _dev(x, "block_fused")
    _dev(attn_out, "block_fused")
    M, E = x.shape
    if scratch is None:
        scratch = torch.empty(int(load().mst_block_fused_scratch_bytes()), dtype=torch.uint8, device=x.device)
    _check(load().mst_block_fused(ptr(x), ptr(attn_out), ptr(xn_out), dt_of(attn_out), ptr(proj_pack), ptr(proj_bf), ptr(wpack),
                                  ptr(b1f), ptr(b2f), ptr(scratch), scratch.numel(), M, E, eps, stream_of(x)), "mst_block_fused")


def block_fused_s(x: torch.Tensor, attn_out: torch.Tensor, block_seq: torch.Tensor, b1f: torch.Tensor, proj_bf: torch.Tensor,
                  b2f: torch.Tensor, xn_out: Optional[torch.Tensor], eps: float = 1e-6, layout: int = 0):
    """mst_block_fused_s (single-role form of mst_block_fused): x [M,384] fp32 in place += ls1*proj(attn_out) then += the fused
    MLP; xn_out (may be attn_out itself) receives normalise(x_new).  block_seq / b1f / proj_bf / b2f from pack_block_seq."""
    _dev(x, "block_fused_s")
    _dev(attn_out, "block_fused_s")
    M, E = x.shape
    _whole_groups("block_fused_s", M, E, x=x if layout & (LAYOUT_X_IN_IMAGE | LAYOUT_X_OUT_IMAGE) else None,
                  attn_out=attn_out if layout & LAYOUT_ACT_BLOCKED else None, xn_out=xn_out if layout & LAYOUT_ACT_BLOCKED else None)
    _check(load().mst_block_fused_s(ptr(x), ptr(attn_out), ptr(xn_out), dt_of(attn_out), ptr(block_seq), ptr(b1f), ptr(proj_bf),
                                    ptr(b2f), M, E, eps, layout, stream_of(x)), "mst_block_fused_s")


LAYOUT_X_IN_IMAGE, LAYOUT_X_OUT_IMAGE, LAYOUT_ACT_BLOCKED = 1, 2, 4


def to_blocked16(a: torch.Tensor) -> torch.Tensor:
    """Row-major [M, C] (M % 32 == 0, C % 16 == 0) -> the 16-bit "blocked" layout of include/mst_hip.h (test / tooling helper)."""
    M, Cn = a.shape
    return a.reshape(M // 32, 32, Cn // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().reshape(M, Cn)


def from_blocked16(a: torch.Tensor) -> torch.Tensor:
    M, Cn = a.shape
    return a.reshape(M // 32, Cn // 16, 2, 32, 8).permute(0, 3, 1, 2, 4).contiguous().reshape(M, Cn)


def to_image32(a: torch.Tensor) -> torch.Tensor:
    """Row-major fp32 [M, C] (M % 32 == 0, C % 8 == 0) -> the fp32 "image" layout of include/mst_hip.h."""
    M, Cn = a.shape
    return a.reshape(M // 32, 32, Cn // 8, 2, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(M, Cn)


def from_image32(a: torch.Tensor) -> torch.Tensor:
    M, Cn = a.shape
    return a.reshape(M // 32, Cn // 8, 2, 32, 4).permute(0, 3, 1, 2, 4).contiguous().reshape(M, Cn)


def pack_block_seq(proj_w, proj_b, ls1, fc1_w, fc1_b, fc2_w, fc2_b, ln_w, ln_b, ls2, dtype: torch.dtype):
    """Host-side packing of one block's out-projection + MLP weights for mst_block_fused_s (layout: include/mst_hip.h): one
    stream of 108 x 24 KiB elements in the order the kernel consumes them, every element 24 MFMA A-fragments in lane order.
    LayerNorm2's affine is folded into fc1, LayerScale into proj / fc2 (layer_scale.py:26-27).  Inputs fp32 (any device):
    proj_w [384,384], proj_b [384], fc1_w [1536,384], fc1_b [1536], fc2_w [384,1536], fc2_b [384], ln_w / ln_b [384], ls1 /
    ls2 [384] or None.  Returns (block_seq [108, 12288] dtype, b1f [1536] fp32, proj_bf [384] fp32, b2f [384] fp32)."""
    dev = proj_w.device
    wp = proj_w.float()
    pbf = proj_b.float().clone()
    if ls1 is not None:
        wp = wp * ls1.float()[:, None]
        pbf = pbf * ls1.float()
    w1 = fc1_w.float() * ln_w.float()[None, :]
    b1f = fc1_b.float() + (fc1_w.float() * ln_b.float()[None, :]).sum(dim=1)      # (weight preparation without a vendor BLAS call)
    w2 = fc2_w.float()
    b2f = fc2_b.float().clone()
    if ls2 is not None:
        w2 = w2 * ls2.float()[:, None]
        b2f = b2f * ls2.float()
    ar = lambda n: torch.arange(n, device=dev)
    lane = ar(64)
    m, h = (lane & 31)[None, None, :, None], (lane >> 5)[None, None, :, None]          # [t, p, lane, e]
    t, p, e = ar(12)[:, None, None, None], ar(2)[None, :, None, None], ar(8)[None, None, None, :]
    k8 = 16 * p + 8 * (e >> 2) + 4 * h + (e & 3)                                       # accumulator-tile k order within 32
    rows_t = (32 * t + m).expand(12, 2, 64, 8)
    # out-projection chunk j: Wp[32t+m][32j + 16p + 8h + e]
    kp = (16 * p + 8 * h + e).expand(12, 2, 64, 8)
    proj = torch.stack([wp[rows_t, 32 * j + kp] for j in range(12)])                   # [12, t, p, lane, e]
    # W1 chunk c, fragment = k-step 2t+p: W1[32c+m][32t + k8]
    cols1 = (32 * t + k8).expand(12, 2, 64, 8)
    rows1 = m.expand(12, 2, 64, 8)
    w1c = torch.stack([w1[32 * c + rows1, cols1] for c in range(48)])                  # [48, t, p, lane, e]
    # W2 chunk c, fragment 2t+p: W2[32t+m][32c + k8]
    k2 = k8.expand(12, 2, 64, 8)
    w2c = torch.stack([w2[rows_t, 32 * c + k2] for c in range(48)])
    proj, w1c, w2c = proj.reshape(12, -1), w1c.reshape(48, -1), w2c.reshape(48, -1)
    seq = [proj, w1c[0:1]]
    inter = torch.stack([w1c[1:48], w2c[0:47]], dim=1).reshape(94, -1)                 # W1(c+1), W2(c) for c = 0..46
    seq += [inter, w2c[47:48]]
    block_seq = torch.cat(seq, dim=0).to(dtype).contiguous()
    assert block_seq.shape == (108, 12288)
    return block_seq, b1f.contiguous(), pbf.contiguous(), b2f.contiguous()


def _w2_row_order(dev):
    R = torch.arange(384, device=dev)
    t, i = R >> 4, R & 15
    nphys = 32 * (t >> 1) + 8 * (i >> 2) + 4 * (t & 1) + (i & 3)          # accumulator row R holds output column n(R)
    cidx = torch.arange(4, device=dev)[None, :] ^ ((-(R >> 2)) & 3)[:, None]   # [R, slot] -> 16-byte chunk (bank swizzle)
    return R, nphys, cidx


def pack_proj(proj_w, proj_b, ls1, dtype: torch.dtype):
    """Host-side packing of the attention out-projection for mst_block_fused (layout: include/mst_hip.h).  proj_w [384,384],
    proj_b [384], ls1 [384] or None (LayerScale folded: layer_scale.py:26-27).  Returns (proj_pack [12, 12288] dtype,
    proj_bf [384] fp32)."""
    dev = proj_w.device
    w = proj_w.float()
    b = proj_b.float().clone()
    if ls1 is not None:
        w = w * ls1.float()[:, None]
        b = b * ls1.float()
    R, nphys, cidx = _w2_row_order(dev)
    wc = w[nphys].view(384, 12, 4, 8).permute(1, 0, 2, 3)                   # [chunk, R, c, j]: natural k order inside a chunk
    img = wc[:, R[:, None], cidx, :]                                        # [chunk, R, slot, 8]
    return img.reshape(12, -1).to(dtype).contiguous(), b.contiguous()


def pack_mlp(fc1_w, fc1_b, fc2_w, fc2_b, ln_w, ln_b, ls2, dtype: torch.dtype):
    """Host-side packing of one MLP for mst_mlp_fused (layout: include/mst_hip.h).  Inputs fp32 tensors on any
    device: fc1_w [1536,384], fc1_b [1536], fc2_w [384,1536], fc2_b [384], ln_w/ln_b [384], ls2 [384] or None.
    Returns (wpack [48,24576] dtype, b1f [1568] fp32, b2f [384] fp32)."""
    dev = fc1_w.device
    w1f = fc1_w.float() * ln_w.float()[None, :]
    b1f = fc1_b.float() + (fc1_w.float() * ln_b.float()[None, :]).sum(dim=1)      # (weight preparation without a vendor BLAS call)
    b2f = fc2_b.float().clone()
    if ls2 is not None:                                   # LayerScale folded into fc2 (layer_scale.py:26-27)
        fc2_w = fc2_w.float() * ls2.float()[:, None]
        b2f = b2f * ls2.float()
    ar = lambda n: torch.arange(n, device=dev)
    # W1 image: [chunk][ks][h][slot][8]
    w1c = w1f.view(48, 32, 12, 4, 8).permute(0, 2, 1, 3, 4)                    # [chunk, ks, h, c, j]
    fh = (-(ar(32) >> 2)) & 3
    cidx = ar(4)[None, :] ^ fh[:, None]                                         # [h, slot] -> c
    w1img = w1c[:, :, ar(32)[:, None], cidx, :]                                 # [chunk, ks, h, slot, 8]
    # W2 image: [chunk][R][slot][8]
    p = ar(32); c = p >> 3; j = p & 7
    phys = torch.where(j < 4, 4 * c + j, 16 + 4 * c + j - 4)
    R = ar(384); t = R >> 4; i = R & 15
    nphys = 32 * (t >> 1) + 8 * (i >> 2) + 4 * (t & 1) + (i & 3)
    w2p = fc2_w.float().view(384, 48, 32)[:, :, phys][nphys]                    # [R, chunk, p]
    w2c = w2p.permute(1, 0, 2).reshape(48, 384, 4, 8)                           # [chunk, R, c, j]
    fR = (-(R >> 2)) & 3
    cidxR = ar(4)[None, :] ^ fR[:, None]
    w2img = w2c[:, R[:, None], cidxR, :]                                        # [chunk, R, slot, 8]
    wpack = torch.cat([w1img.reshape(48, -1), w2img.reshape(48, -1)], dim=1).to(dtype).contiguous()
    b1p = torch.zeros(1536 + 32, device=dev, dtype=torch.float32)
    b1p[:1536] = b1f
    return wpack, b1p, b2f.contiguous()


def swiglu_hidden(embed_dim: int) -> int:
    """Hidden width of SwiGLUFFNFused(E, 4E) (swiglu_ffn.py:63-64): (int(4E * 2 / 3) + 7) // 8 * 8."""
    return (int(4 * embed_dim * 2 / 3) + 7) // 8 * 8


def swiglu_group(dtype: torch.dtype) -> int:
    """Pairing group of the MST_EPI_BIAS_SWIGLU weight image per operand type (include/mst_hip.h, mst_gemm)."""
    return 32 if dtype == torch.float32 else 16


def pack_swiglu(w12, b12, w3, dtype: torch.dtype):
    """Weight images of one SwiGLUFFNFused for MST_EPI_BIAS_SWIGLU (layout: include/mst_hip.h, mst_gemm).  w12 [2H, E], b12 [2H],
    w3 [E, H] on any device (the model packs on the GPU, once per weight version).  H is padded with zero rows to Hp, a multiple of 64:
    zero gate rows give zero hidden columns, which meet zero w3 columns.  Returns (w12p [2 Hp, E] dtype, gate and value rows interleaved
    in groups of swiglu_group(dtype); b12p [2 Hp] fp32, paired the same way; w3p [E, Hp] dtype)."""
    H2, E = w12.shape
    H = H2 // 2
    if H2 != 2 * H or tuple(b12.shape) != (H2,) or tuple(w3.shape) != (E, H):
        raise ValueError(f"pack_swiglu: w12 {tuple(w12.shape)}, b12 {tuple(b12.shape)}, w3 {tuple(w3.shape)} are not [2H, E], [2H], [E, H]")
    G = swiglu_group(dtype)
    Hp = (H + 63) // 64 * 64
    dev = w12.device
    wg = torch.zeros((2, Hp, E), dtype=torch.float32, device=dev)
    wg[:, :H] = w12.detach().float().view(2, H, E)
    bg = torch.zeros((2, Hp), dtype=torch.float32, device=dev)
    bg[:, :H] = b12.detach().float().view(2, H)
    w12p = wg.view(2, Hp // G, G, E).permute(1, 0, 2, 3).reshape(2 * Hp, E).to(dtype).contiguous()
    b12p = bg.view(2, Hp // G, G).permute(1, 0, 2).reshape(2 * Hp).contiguous()
    w3p = torch.zeros((E, Hp), dtype=torch.float32, device=dev)
    w3p[:, :H] = w3.detach().float()
    return w12p, b12p, w3p.to(dtype).contiguous()


def vit_workspace_bytes(w: VitWeights, H: int, W: int, chunk: int) -> int:
    return int(load().mst_vit_workspace_bytes(C.byref(w), H, W, chunk))


def vit_encode(w: VitWeights, vol: torch.Tensor, cls_out: torch.Tensor, cls_probs: Optional[torch.Tensor],
               n_layers_probs: int, chunk: int, ws: torch.Tensor, full_probs: Optional[torch.Tensor] = None):
    _dev(vol, "vit_encode")
    n, H, W = vol.shape
    _check(load().mst_vit_encode(C.byref(w), ptr(vol), dt_of(vol), n, H, W, ptr(cls_out), ptr(cls_probs),
                                 ptr(full_probs), n_layers_probs, chunk, ptr(ws), ws.numel() * ws.element_size(),
                                 stream_of(vol)), "mst_vit_encode")


def vit_features_workspace_bytes(w: VitWeights, in_channels: int, H: int, W: int, chunk: int) -> int:
    return int(load().mst_vit_features_workspace_bytes(C.byref(w), in_channels, H, W, chunk))


def pack_patch_rgb(weight: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Conv2d(3, E, 14, 14).weight -> the [E, 3*14*16] image mst_vit_encode_features reads as patch_w_rgb: every kernel row padded
    to 16 columns with zeros (K = 588 -> 672), in the compute dtype."""
    E = weight.shape[0]
    wp = torch.zeros((E, 3, 14, 16), dtype=torch.float32, device=weight.device)
    wp[..., :14] = weight.detach().float()
    return wp.reshape(E, 3 * 14 * 16).to(dtype).contiguous()


def vit_encode_features(w: VitWeights, img: torch.Tensor, chunk: int, ws: torch.Tensor, *, patch_w_rgb: Optional[torch.Tensor] = None,
                        cls_out: Optional[torch.Tensor] = None, blocks: Sequence[int] = (), norm: bool = True,
                        out: Optional[torch.Tensor] = None):
    """mst_vit_encode_features.  img [n, H, W] (grey) or [n, 3, H, W] (RGB, with patch_w_rgb from pack_patch_rgb).  cls_out
    (optional) fp32 [n, E].  blocks (strictly ascending block indices) with out fp32 [len(blocks), n, N, E] contiguous: the residual
    stream behind those blocks, through encoder.norm when `norm`.  `out` may be a view into a larger tensor; exactly its elements
    are written."""
    _dev(img, "vit_encode_features")
    if img.dim() == 4:
        n, ch, H, W = img.shape
    else:
        (n, H, W), ch = img.shape, 1
    if ch == 3 and patch_w_rgb is None:
        raise ValueError("vit_encode_features: RGB input needs patch_w_rgb")
    taps = None
    blocks = [int(b) for b in blocks]
    if blocks:
        N = 1 + w.num_registers + (H // 14) * (W // 14)
        if out is None or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() \
                or tuple(out.shape) != (len(blocks), n, N, w.embed_dim):
            raise ValueError(f"vit_encode_features: out must be a contiguous fp32 device tensor of shape {(len(blocks), n, N, w.embed_dim)}")
        idx = (_i * len(blocks))(*blocks)
        taps = VitTaps(len(blocks), idx, 1 if norm else 0, ptr(out))
    _check(load().mst_vit_encode_features(C.byref(w), ptr(img), dt_of(img), ch, n, H, W, ptr(patch_w_rgb), ptr(cls_out),
                                          None if taps is None else C.byref(taps), chunk, ptr(ws), ws.numel() * ws.element_size(),
                                          stream_of(img)), "mst_vit_encode_features")


def fusion_workspace_bytes(w: FusionWeights, B: int, D: int) -> int:
    return int(load().mst_fusion_workspace_bytes(C.byref(w), B, D))


def slice_fusion(w: FusionWeights, emb: torch.Tensor, B: int, D: int, mask: Optional[torch.Tensor],
                 features: torch.Tensor, logits: Optional[torch.Tensor], slice_probs: Optional[torch.Tensor],
                 ws: torch.Tensor):
    _dev(emb, "slice_fusion")
    _check(load().mst_slice_fusion(C.byref(w), ptr(emb), B, D, ptr(mask), ptr(features), ptr(logits), ptr(slice_probs),
                                   ptr(ws), ws.numel() * ws.element_size(), stream_of(emb)), "mst_slice_fusion")


def attention_readout(cls_probs_last: Optional[torch.Tensor], slice_probs: Optional[torch.Tensor], B: int, D: int,
                      heads: int, N: int, num_registers: int, sheads: int, plane: Optional[torch.Tensor],
                      slice_attn: Optional[torch.Tensor], maps: Optional[torch.Tensor]):
    t = cls_probs_last if cls_probs_last is not None else slice_probs
    _check(load().mst_attention_readout(ptr(cls_probs_last), ptr(slice_probs), B, D, heads, N, num_registers, sheads,
                                        ptr(plane), ptr(slice_attn), ptr(maps), stream_of(t)), "mst_attention_readout")


def saliency_accumulate(maps: torch.Tensor, slice_attn: Optional[torch.Tensor], gh: int, gw: int, flip_mask: int,
                        lowres: torch.Tensor, slice_acc: Optional[torch.Tensor], accumulate: bool):
    """lowres [D,gh,gw] (+)= head-mean of maps [D,heads,Np], TTA flips (bit 0 depth, 1 height, 2 width) mirrored back."""
    _dev(maps, "saliency_accumulate")
    D, heads, Np = maps.shape
    _check(load().mst_saliency_accumulate(ptr(maps), ptr(slice_attn), D, heads, gh, gw, Np, flip_mask, 1 if accumulate else 0,
                                          ptr(lowres), ptr(slice_acc), stream_of(maps)), "mst_saliency_accumulate")


def saliency_upsample(lowres: torch.Tensor, size, scale: float = 1.0) -> torch.Tensor:
    """scale * F.interpolate(lowres[None, None], size, mode='trilinear') -> [Dout, H, W] fp32."""
    _dev(lowres, "saliency_upsample")
    D, gh, gw = lowres.shape
    Dout, H, W = (int(v) for v in size)
    out = torch.empty((Dout, H, W), dtype=torch.float32, device=lowres.device)
    _check(load().mst_saliency_upsample(ptr(lowres), D, gh, gw, float(scale), Dout, H, W, ptr(out), stream_of(lowres)),
           "mst_saliency_upsample")
    return out


def tta_inplane_flips(x: torch.Tensor) -> torch.Tensor:
    """mst_tta_inplane_flips: slices x [n, H, W] (fp32 / fp16 / bf16) -> [4, n, H, W] of x's type: x, torch.flip(x, (1,)),
    torch.flip(x, (2,)), torch.flip(x, (1, 2)) -- the in-plane halves of the script's eight TTA flips (main_predict.py:147-158)."""
    _operand(x, "tta_inplane_flips", "x", (torch.float32,) + _T16)
    if x.dim() != 3 or 0 in x.shape:
        raise ValueError(f"tta_inplane_flips: x must be [n, H, W] and not empty, got {list(x.shape)}")
    _resident("tta_inplane_flips", x=x)
    n, H, W = x.shape
    out = torch.empty((4, n, H, W), dtype=x.dtype, device=x.device)
    _check(load().mst_tta_inplane_flips(ptr(x), dt_of(x), n, H, W, ptr(out), stream_of(x)), "mst_tta_inplane_flips")
    return out


def saliency_accumulate_tta(plane: torch.Tensor, slice_attn: torch.Tensor, gh: int, gw: int, lowres: torch.Tensor,
                            slice_acc: Optional[torch.Tensor]):
    """mst_saliency_accumulate_tta: lowres [D,gh,gw] = the eight-variant TTA sum of head-mean(plane [4,D,heads,Np]) * slice_attn [8,D],
    flips mirrored back; slice_acc [D] (optional) = the sum of slice_attn alone.  Overwrites; fixed summation order."""
    _operand(plane, "saliency_accumulate_tta", "plane", (torch.float32,))
    if plane.dim() != 4 or plane.shape[0] != 4 or 0 in plane.shape:
        raise ValueError(f"saliency_accumulate_tta: plane must be [4, D, heads, Np] and not empty, got {list(plane.shape)}")
    _, D, heads, Np = plane.shape
    if gh < 1 or gw < 1 or gh * gw > Np:
        raise ValueError(f"saliency_accumulate_tta: grid {gh} x {gw} does not fit {Np} map columns")
    _operand(slice_attn, "saliency_accumulate_tta", "slice_attn", (torch.float32,), (8, D))
    _operand(lowres, "saliency_accumulate_tta", "lowres", (torch.float32,), (D, gh, gw))
    if slice_acc is not None:
        _operand(slice_acc, "saliency_accumulate_tta", "slice_acc", (torch.float32,), (D,))
    _resident("saliency_accumulate_tta", plane=plane, slice_attn=slice_attn, lowres=lowres, slice_acc=slice_acc)
    _check(load().mst_saliency_accumulate_tta(ptr(plane), ptr(slice_attn), D, heads, gh, gw, Np, ptr(lowres), ptr(slice_acc),
                                              stream_of(plane)), "mst_saliency_accumulate_tta")


def liere_rotation(vars_: Sequence[torch.Tensor]) -> torch.Tensor:
    """AttentionLiereRotator's rotation R [hd, hd] from its ParameterList (each [n(n-1)/2, axes_length, 1])."""
    v = torch.stack([t.detach().float().reshape(t.shape[0], t.shape[1]) for t in vars_]).contiguous()
    _dev(v, "liere_rotation")
    nb, m, P = v.shape
    n = int(round((1 + (1 + 8 * m) ** 0.5) / 2))
    if n * (n - 1) // 2 != m:
        raise ValueError(f"liere_rotation: {m} parameters per block is not n(n-1)/2")
    R = torch.empty((nb * n, nb * n), dtype=torch.float32, device=v.device)
    _check(load().mst_liere_rotation(ptr(v), nb, n, P, ptr(R), stream_of(v)), "mst_liere_rotation")
    return R


def attention_rollout(maps: Sequence[torch.Tensor]) -> torch.Tensor:
    """get_attention_cls (dino.py:204-212): maps[0] @ maps[1] @ ... @ maps[-1] on full fp32 [..., N, N] maps."""
    m0 = maps[0]
    _dev(m0, "attention_rollout")
    N = m0.shape[-1]
    for m in maps:
        if m.dtype != torch.float32 or tuple(m.shape) != tuple(m0.shape) or m.shape[-2] != N or not m.is_contiguous():
            raise ValueError("attention_rollout: maps must be contiguous fp32 [..., N, N] tensors of one shape")
    batch = m0.numel() // (N * N)
    out = torch.empty_like(m0)
    tmp = torch.empty_like(m0) if len(maps) > 2 else None
    arr = (_vp * len(maps))(*[ptr(m) for m in maps])
    _check(load().mst_attention_rollout(arr, len(maps), batch, N, ptr(out), ptr(tmp), stream_of(m0)),
           "mst_attention_rollout")
    return out


# ---- training-step ops (fp32; orchestrated by mst/train.py) ---------------------------------------------------------
def gemm_ex(A: torch.Tensor, B: torch.Tensor, C: torch.Tensor, M: int, N: int, K: int, sa, sb, sc, nb=(1, 1),
            ba=(0, 0), bb=(0, 0), bc=(0, 0), alpha: float = 1.0, beta: float = 0.0, offs=(0, 0, 0)):
    """C[b] = alpha * A[b] . B[b] + beta * C[b]; sa = (A_m, A_k), sb = (B_k, B_n), sc = (C_m, C_n) element strides, nb = (nb1, nb2),
    ba / bb / bc = per-level batch strides, offs = element offsets of A, B, C into their tensors (views without copies)."""
    st = (_i64 * 12)(sa[0], sa[1], sb[0], sb[1], sc[0], sc[1], ba[0], ba[1], bb[0], bb[1], bc[0], bc[1])
    _check(load().mst_gemm_ex(A.data_ptr() + 4 * offs[0], B.data_ptr() + 4 * offs[1], C.data_ptr() + 4 * offs[2], M, N, K, st,
                              nb[0], nb[1], alpha, beta, stream_of(C)), "mst_gemm_ex")
    return C


def cvt16(x: torch.Tensor, dtype: torch.dtype, *, transpose: bool = False, rows_pad: Optional[int] = None, scale: float = 1.0) -> torch.Tensor:
    """mst_cvt16: the 16-bit image of an fp32 matrix [rows, cols] -- the same layout, or transposed [cols, rows_pad] with zero columns for
    rows .. rows_pad (operands of the mixed-precision training GEMMs)."""
    _dev(x, "cvt16")
    rows, cols = x.shape
    if transpose:
        rp = rows_pad or rows
        out = torch.empty((cols, rp), dtype=dtype, device=x.device)
        _check(load().mst_cvt16(ptr(x), cols, rows, cols, scale, ptr(out), dt_of(out), rp, 1, rp, stream_of(x)), "mst_cvt16")
        return out
    out = torch.empty((rows, cols), dtype=dtype, device=x.device)
    _check(load().mst_cvt16(ptr(x), cols, rows, cols, scale, ptr(out), dt_of(out), cols, 0, rows, stream_of(x)), "mst_cvt16")
    return out


def gemm16_splitk(a: torch.Tensor, w: torch.Tensor, splits: int) -> torch.Tensor:
    """mst_gemm16_splitk: partial products [splits, M, N] fp32 of a [M, K] . w [N, K]^T over `splits` equal K ranges (16-bit operands)."""
    _dev(a, "gemm16_splitk")
    _dev(w, "gemm16_splitk")
    M, K = a.shape
    N = w.shape[0]
    part = torch.empty((splits, M, N), dtype=torch.float32, device=a.device)
    _check(load().mst_gemm16_splitk(ptr(a), dt_of(a), K, ptr(w), K, ptr(part), N, M, N, K, splits, M * N, stream_of(a)), "mst_gemm16_splitk")
    return part


def rope_rows(qkv: torch.Tensor, L: int, heads: int, hd: int, freqs: torch.Tensor, sign: float = 1.0) -> torch.Tensor:
    """mst_rope_rows: rotate the q and k pairs of packed rows [rows, 3*heads*hd] in place (sign -1: the adjoint, for gradient rows)."""
    _dev(qkv, "rope_rows")
    _check(load().mst_rope_rows(ptr(qkv), qkv.shape[0], L, heads, hd, ptr(freqs), sign, stream_of(qkv)), "mst_rope_rows")
    return qkv


def softmax_rows(S: torch.Tensor, mask: Optional[torch.Tensor], rows_per_batch: int):
    L = S.shape[-1]
    _check(load().mst_softmax_rows(ptr(S), ptr(mask), S.numel() // L, L, rows_per_batch, stream_of(S)), "mst_softmax_rows")
    return S


def softmax_rows_bwd(P: torch.Tensor, dP: torch.Tensor, scale: float = 1.0):
    L = P.shape[-1]
    _check(load().mst_softmax_rows_bwd(ptr(P), ptr(dP), P.numel() // L, L, scale, stream_of(P)), "mst_softmax_rows_bwd")
    return dP


def layernorm_rows(x: torch.Tensor, x_stride: int, rows: int, cols: int, weight, bias, eps: float) -> torch.Tensor:
    """LayerNorm of `rows` rows of `cols` fp32 values starting at x's first element, row stride x_stride -> [rows, cols] fp32."""
    out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    _check(load().mst_layernorm(ptr(x), x_stride, ptr(weight), ptr(bias), ptr(out), F32, cols, rows, cols, eps, stream_of(x)),
           "mst_layernorm")
    return out


def layernorm_bwd(x, x_stride, gamma, dy, dy_stride, dres, dres_stride, dx, dx_stride, dgamma, dbeta, rows, cols, eps):
    if deterministic():
        _call_ws("mst_layernorm_bwd_ordered", (rows, cols), x, ptr(x), x_stride, ptr(gamma), ptr(dy), dy_stride, ptr(dres), dres_stride,
                 ptr(dx), dx_stride, ptr(dgamma), ptr(dbeta), rows, cols, eps)
        return
    _check(load().mst_layernorm_bwd(ptr(x), x_stride, ptr(gamma), ptr(dy), dy_stride, ptr(dres), dres_stride, ptr(dx), dx_stride,
                                    ptr(dgamma), ptr(dbeta), rows, cols, eps, stream_of(x)), "mst_layernorm_bwd")


def act_fwd(h: torch.Tensor, kind: int) -> torch.Tensor:
    """mst_act_fwd / mst_act_fwd16 by h's dtype: act(h) in h's dtype (kind 0: GELU, 1: ReLU)."""
    y = torch.empty_like(h)
    if h.dtype == torch.float32:
        _check(load().mst_act_fwd(ptr(h), ptr(y), h.numel(), kind, stream_of(h)), "mst_act_fwd")
    else:
        _check(load().mst_act_fwd16(ptr(h), ptr(y), dt_of(h), h.numel(), kind, stream_of(h)), "mst_act_fwd16")
    return y


def act_bwd(h: torch.Tensor, dy: torch.Tensor, kind: int) -> torch.Tensor:
    """mst_act_bwd / mst_act_bwd16 by h's dtype: dy (fp32, in place) *= act'(h)."""
    if h.dtype == torch.float32:
        _check(load().mst_act_bwd(ptr(h), ptr(dy), h.numel(), kind, stream_of(h)), "mst_act_bwd")
    else:
        _check(load().mst_act_bwd16(ptr(h), dt_of(h), ptr(dy), h.numel(), kind, stream_of(h)), "mst_act_bwd16")
    return dy


def swiglu_fwd(x12: torch.Tensor) -> torch.Tensor:
    """mst_swiglu_fwd / mst_swiglu_fwd16 by x12's dtype: h = silu(x1) * x2 of x12 = [x1 | x2] ([rows, 2H] -> [rows, H], x12's dtype)."""
    _dev(x12, "swiglu_fwd")
    rows, H2 = x12.shape
    if H2 % 2:
        raise ValueError("swiglu_fwd: x12 must have an even number of columns")
    h = torch.empty((rows, H2 // 2), dtype=x12.dtype, device=x12.device)
    if x12.dtype == torch.float32:
        _check(load().mst_swiglu_fwd(ptr(x12), ptr(h), rows, H2 // 2, stream_of(x12)), "mst_swiglu_fwd")
    else:
        _check(load().mst_swiglu_fwd16(ptr(x12), ptr(h), dt_of(x12), rows, H2 // 2, stream_of(x12)), "mst_swiglu_fwd16")
    return h


def swiglu_bwd(x12: torch.Tensor, dh: torch.Tensor) -> torch.Tensor:
    """mst_swiglu_bwd / mst_swiglu_bwd16 by x12's dtype: the fp32 gradient [rows, 2H] of x12 from dh fp32 [rows, H]."""
    _dev(x12, "swiglu_bwd")
    _dev(dh, "swiglu_bwd")
    rows, H2 = x12.shape
    if dh.dtype != torch.float32 or tuple(dh.shape) != (rows, H2 // 2) or H2 % 2 or dh.device != x12.device:
        raise ValueError("swiglu_bwd: dh must be fp32 [rows, H] on x12's device for x12 [rows, 2H]")
    dx = torch.empty((rows, H2), dtype=torch.float32, device=x12.device)
    if x12.dtype == torch.float32:
        _check(load().mst_swiglu_bwd(ptr(x12), ptr(dh), ptr(dx), rows, H2 // 2, stream_of(x12)), "mst_swiglu_bwd")
    else:
        _check(load().mst_swiglu_bwd16(ptr(x12), dt_of(x12), ptr(dh), ptr(dx), rows, H2 // 2, stream_of(x12)), "mst_swiglu_bwd16")
    return dx


def _is16(t: torch.Tensor, what: str, name: str):
    if t.dtype not in (torch.bfloat16, torch.float16):
        raise TypeError(f"{what}: {name} must be bf16 or fp16 (got {t.dtype})")
    _dev(t, what)


def residual_layernorm16(x_in: torch.Tensor, br: torch.Tensor, gamma: Optional[torch.Tensor], ln_w: Optional[torch.Tensor],
                         ln_b: Optional[torch.Tensor], eps: float, x_out: Optional[torch.Tensor] = None,
                         y: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """mst_residual_layernorm16: (x_out fp32 = x_in + gamma * br, y = LayerNorm(x_out; ln_w, ln_b) in br's 16-bit type) in one pass over
    [rows, cols]; gamma None: no LayerScale; ln_w None: the residual alone, y is None.  x_out / y: caller-given outputs (every element
    is written)."""
    what = "residual_layernorm16"
    _dev(x_in, what)
    _is16(br, what, "br")
    if x_in.dtype != torch.float32 or x_in.dim() != 2 or br.shape != x_in.shape or br.device != x_in.device:
        raise ValueError(f"{what}: x_in must be fp32 [rows, cols] and br a 16-bit tensor of that shape on its device")
    rows, cols = x_in.shape
    if x_out is None:
        x_out = torch.empty_like(x_in)
    if ln_w is None:
        y = None
    elif y is None:
        y = torch.empty_like(br)
    for t, like, name in ((x_out, x_in, "x_out"), (y, br, "y")):
        if t is not None and (t.dtype != like.dtype or t.shape != like.shape or t.device != like.device or not t.is_contiguous()):
            raise ValueError(f"{what}: {name} must be contiguous {like.dtype} {tuple(like.shape)} on {like.device}")
    _check(load().mst_residual_layernorm16(ptr(x_in), ptr(br), dt_of(br), ptr(gamma), ptr(x_out), ptr(ln_w), ptr(ln_b), ptr(y), rows, cols,
                                           eps, stream_of(x_in)), "mst_residual_layernorm16")
    return x_out, y


def act_fwd16(h: torch.Tensor, kind: int) -> torch.Tensor:
    """mst_act_fwd16: act(h) of a 16-bit tensor in its own type (fp32 arithmetic, one rounding)."""
    _is16(h, "act_fwd16", "h")
    y = torch.empty_like(h)
    _check(load().mst_act_fwd16(ptr(h), ptr(y), dt_of(h), h.numel(), kind, stream_of(h)), "mst_act_fwd16")
    return y


def act_bwd16(h: torch.Tensor, dy: torch.Tensor, kind: int) -> torch.Tensor:
    """mst_act_bwd16: dy (fp32, in place) *= act'(h) with the pre-activation h in 16 bits."""
    _is16(h, "act_bwd16", "h")
    _dev(dy, "act_bwd16")
    if dy.dtype != torch.float32 or dy.numel() != h.numel() or dy.device != h.device:
        raise ValueError("act_bwd16: dy must be fp32 with h's element count on its device")
    _check(load().mst_act_bwd16(ptr(h), dt_of(h), ptr(dy), h.numel(), kind, stream_of(h)), "mst_act_bwd16")
    return dy


def transpose16(x: torch.Tensor, rows_pad: Optional[int] = None) -> torch.Tensor:
    """mst_transpose16: the transposed image [cols, rows_pad] of a 16-bit matrix [rows, cols], zero columns for rows .. rows_pad."""
    _is16(x, "transpose16", "x")
    rows, cols = x.shape
    rp = rows_pad or rows
    out = torch.empty((cols, rp), dtype=x.dtype, device=x.device)
    _check(load().mst_transpose16(ptr(x), dt_of(x), cols, rows, cols, ptr(out), rp, rp, stream_of(x)), "mst_transpose16")
    return out


def colsum(a: torch.Tensor, out: torch.Tensor, b: Optional[torch.Tensor] = None):
    """out[c] += sum_r a[r][c] * (b ? b[r][c] : 1); a (and b) 2-D with unit column stride (any row stride: a column block of a wider
    matrix), out contiguous.  b may be bf16 / fp16 (the 16-bit storage mode's saved branch output)."""
    rows, cols = a.shape
    if a.stride(1) != 1 or (b is not None and (b.shape != a.shape or b.stride(1) != 1)) or not out.is_contiguous():
        raise ValueError("colsum: a / b need unit column strides and equal shapes, out must be contiguous")
    as_ = a.stride(0) if rows > 1 else cols
    bs = (b.stride(0) if rows > 1 else cols) if b is not None else cols
    if b is not None and b.dtype != torch.float32:       # a factor saved in 16 bits (train_storage='16bit'): mst_colsum_b16 / _ordered
        if deterministic():
            _call_ws("mst_colsum_b16_ordered", (rows, cols), a, ptr(a), as_, ptr(b), dt_of(b), bs, rows, cols, ptr(out),
                     sized_by="mst_colsum_ordered")
        else:
            _check(load().mst_colsum_b16(ptr(a), as_, ptr(b), dt_of(b), bs, rows, cols, ptr(out), stream_of(a)), "mst_colsum_b16")
        return out
    if deterministic():
        _call_ws("mst_colsum_ordered", (rows, cols), a, ptr(a), as_, ptr(b), bs, rows, cols, ptr(out))
        return out
    _check(load().mst_colsum(ptr(a), as_, ptr(b), bs, rows, cols, ptr(out), stream_of(a)), "mst_colsum")
    return out


def axpby_cols(x: torch.Tensor, y: torch.Tensor, g: Optional[torch.Tensor] = None, alpha: float = 1.0, beta: float = 1.0,
               rows: Optional[int] = None, cols: Optional[int] = None, x_stride: Optional[int] = None, y_stride: Optional[int] = None):
    """y = alpha * x * g + beta * y over [rows, cols] (defaults: x's own 2-D shape, contiguous)."""
    cols = cols if cols is not None else x.shape[-1]
    rows = rows if rows is not None else x.numel() // cols
    _check(load().mst_axpby_cols(ptr(x), x_stride if x_stride is not None else cols, ptr(g), alpha, beta, ptr(y),
                                 y_stride if y_stride is not None else cols, rows, cols, stream_of(x)), "mst_axpby_cols")
    return y


def im2col14(vol: torch.Tensor) -> torch.Tensor:
    n, H, W = vol.shape
    col = torch.empty((n * (H // 14) * (W // 14), 196), dtype=torch.float32, device=vol.device)
    _check(load().mst_im2col14(ptr(vol), dt_of(vol), n, H, W, ptr(col), stream_of(vol)), "mst_im2col14")
    return col


def patch_embed_dgrad(dx: torch.Tensor, wsum: torch.Tensor, n: int, H: int, W: int, tokens: Optional[int] = None, first: int = 0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient with respect to the grey volume [n, H, W] (fp32) of the patch embedding: dx holds the patch-row gradients, row
    s * tokens + first + p for patch p of image s (tokens defaults to the patch count: dx is the patch rows alone), wsum is the
    [E, 14 * 16] channel-summed kernel the forward's mst_patch_embed read.  Every pixel of `out` is written."""
    _dev(dx, "patch_embed_dgrad")
    E = wsum.shape[0]
    Np = (H // 14) * (W // 14)
    tokens = Np if tokens is None else tokens
    if (dx.dtype != torch.float32 or not dx.is_contiguous() or dx.numel() != n * tokens * E or wsum.dtype != torch.float32
            or not wsum.is_contiguous() or tuple(wsum.shape) != (E, 224) or wsum.device != dx.device):
        raise ValueError(f"patch_embed_dgrad: dx must be contiguous fp32 [{n} * {tokens}, E], wsum contiguous fp32 [E, 224] on its device")
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.float32, device=dx.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, H, W) or out.device != dx.device:
        raise ValueError(f"patch_embed_dgrad: out must be contiguous fp32 [{n}, {H}, {W}] on dx's device")
    _check(load().mst_patch_embed_dgrad(ptr(dx), tokens, first, ptr(wsum), n, H, W, E, ptr(out), stream_of(dx)), "mst_patch_embed_dgrad")
    return out


def _rgb_rows(what: str, dx: torch.Tensor, n: int, H: int, W: int, E: int, tokens: Optional[int]) -> int:
    """Tokens per image of the [n * tokens, E] gradient rows `dx` of an RGB patch-embedding gradient (default: the patch rows alone)."""
    _dev(dx, what)
    tokens = (H // 14) * (W // 14) if tokens is None else tokens
    if dx.dtype != torch.float32 or dx.numel() != n * tokens * E:
        raise ValueError(f"{what}: dx must be contiguous fp32 [{n} * {tokens}, {E}]")
    return tokens


def patch_embed_rgb(img: torch.Tensor, wp: torch.Tensor, bias: torch.Tensor, prefix: torch.Tensor, pos_patch: torch.Tensor) -> torch.Tensor:
    """mst_patch_embed_rgb: tokens x fp32 [n, n_prefix + Np, E] of fp32 images [n, 3, H, W]; wp = pack_patch_rgb(weight, torch.float32)."""
    _dev(img, "patch_embed_rgb")
    n, C, H, W = img.shape
    E = wp.shape[0]
    if C != 3 or img.dtype != torch.float32 or wp.dtype != torch.float32 or tuple(wp.shape) != (E, 672) or not wp.is_contiguous():
        raise ValueError("patch_embed_rgb: img must be fp32 [n, 3, H, W], wp the contiguous fp32 [E, 672] image of pack_patch_rgb")
    n_prefix = prefix.shape[0]
    x = torch.empty((n, n_prefix + (H // 14) * (W // 14), E), dtype=torch.float32, device=img.device)
    _check(load().mst_patch_embed_rgb(ptr(img), n, H, W, ptr(wp), ptr(bias), ptr(prefix), n_prefix, ptr(pos_patch), E, ptr(x), stream_of(img)),
           "mst_patch_embed_rgb")
    return x


def patch_embed_rgb_dgrad(dx: torch.Tensor, wp: torch.Tensor, n: int, H: int, W: int, tokens: Optional[int] = None, first: int = 0,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mst_patch_embed_rgb_dgrad: the gradient with respect to the images [n, 3, H, W] (fp32) from the patch-row gradients in dx (rows as
    in `patch_embed_dgrad`); wp is the fp32 [E, 672] kernel image of pack_patch_rgb.  Every pixel of `out` is written once."""
    E = wp.shape[0]
    tokens = _rgb_rows("patch_embed_rgb_dgrad", dx, n, H, W, E, tokens)
    if wp.dtype != torch.float32 or not wp.is_contiguous() or tuple(wp.shape) != (E, 672) or wp.device != dx.device:
        raise ValueError("patch_embed_rgb_dgrad: wp must be the contiguous fp32 [E, 672] image of pack_patch_rgb on dx's device")
    if out is None:
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device=dx.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, 3, H, W) or out.device != dx.device:
        raise ValueError(f"patch_embed_rgb_dgrad: out must be contiguous fp32 [{n}, 3, {H}, {W}] on dx's device")
    _check(load().mst_patch_embed_rgb_dgrad(ptr(dx), tokens, first, ptr(wp), n, H, W, E, ptr(out), stream_of(dx)), "mst_patch_embed_rgb_dgrad")
    return out


def rgb_wgrad_split_rows(rows: int) -> int:
    """Patch rows per partial of mst_patch_embed_rgb_wgrad: 256, or what keeps the partials at 16 (a multiple of the kernel's K-step)."""
    return max(256, -(-rows // (16 * 16)) * 16)


def patch_embed_rgb_wgrad(dx: torch.Tensor, img: torch.Tensor, E: int, tokens: Optional[int] = None, first: int = 0,
                          part: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d weight [E, 3, 14, 14] of the RGB patch embedding from the patch-row gradients in dx and the fp32 images [n, 3, H, W], read in
    place: mst_patch_embed_rgb_wgrad's partials over `rgb_wgrad_split_rows` patch rows each, reduced by `colsum` (atomic, or in fixed
    order under the deterministic flag).  part: the caller's [splits, E * 588] buffer for the partials."""
    _dev(img, "patch_embed_rgb_wgrad")
    n, C, H, W = img.shape
    tokens = _rgb_rows("patch_embed_rgb_wgrad", dx, n, H, W, E, tokens)
    if C != 3 or img.dtype != torch.float32 or img.device != dx.device:
        raise ValueError("patch_embed_rgb_wgrad: img must be fp32 [n, 3, H, W] on dx's device")
    rows = n * (H // 14) * (W // 14)
    chunk = rgb_wgrad_split_rows(rows)
    splits = -(-rows // chunk)
    if part is None:
        part = torch.empty((splits, E * 588), dtype=torch.float32, device=dx.device)
    elif part.dtype != torch.float32 or not part.is_contiguous() or tuple(part.shape) != (splits, E * 588) or part.device != dx.device:
        raise ValueError(f"patch_embed_rgb_wgrad: part must be contiguous fp32 [{splits}, {E * 588}] on dx's device")
    _check(load().mst_patch_embed_rgb_wgrad(ptr(dx), tokens, first, ptr(img), n, H, W, E, chunk, ptr(part), stream_of(dx)),
           "mst_patch_embed_rgb_wgrad")
    return colsum(part, torch.zeros(E * 588, dtype=torch.float32, device=dx.device)).view(E, 3, 14, 14)


def pos_embed_interp_bwd(dout: torch.Tensor, M: int, gh: int, gw: int, offset: float, dpos: torch.Tensor):
    E = dout.shape[-1]
    if deterministic():
        _call_ws("mst_pos_embed_interp_bwd_ordered", (M, E, gh, gw), dout, ptr(dout), M, E, gh, gw, offset, ptr(dpos))
        return dpos
    _check(load().mst_pos_embed_interp_bwd(ptr(dout), M, E, gh, gw, offset, ptr(dpos), stream_of(dout)), "mst_pos_embed_interp_bwd")
    return dpos


# ---- convolutional backbone ops (NHWC fp32) --------------------------------------------------------------------------
def im2col_nhwc(x: torch.Tensor, kh: int, kw: int, stride: int, pad: int, kpad: Optional[int] = None,
                out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """x [n,H,W,C] fp32 -> col [n*Ho*Wo, Kpad] (K = kh*kw*C in (ky,kx,c) order, zero-padded to Kpad), fp32 or rounded to bf16 / fp16."""
    _dev(x, "im2col_nhwc")
    n, H, W, Cc = x.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    K = kh * kw * Cc
    kpad = kpad or (K + 15) // 16 * 16
    col = torch.empty((n * Ho * Wo, kpad), dtype=out_dtype, device=x.device)
    if out_dtype == torch.float32:
        _check(load().mst_im2col_nhwc(ptr(x), n, H, W, Cc, kh, kw, stride, pad, kpad, ptr(col), stream_of(x)), "mst_im2col_nhwc")
    else:
        _check(load().mst_im2col_nhwc16(ptr(x), n, H, W, Cc, kh, kw, stride, pad, kpad, ptr(col), dt_of(col), stream_of(x)), "mst_im2col_nhwc16")
    return col


def conv_gemm(x: torch.Tensor, wg: torch.Tensor, bias: Optional[torch.Tensor], kh: int, kw: int, stride: int, pad: int, *,
              epilogue: int = EPI_BIAS, out: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Convolution of x [n,H,W,Cin] (NHWC fp32, Cin % 16 == 0) with the GEMM-form weight wg [Cout, Kpad] ((ky, kx, c) order) as an
    implicit GEMM (mst_conv_gemm: no im2col matrix) -> [n*Ho*Wo, Cout].  out: the residual operand of EPI_RESIDUAL / EPI_RESIDUAL_RELU (updated in place)."""
    _dev(x, "conv_gemm")
    n, H, W, Cin = x.shape
    Cout, kpad = wg.shape
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty((n * Ho * Wo, Cout), dtype=torch.float32, device=x.device)
    _check(load().mst_conv_gemm(ptr(x), n, H, W, Cin, kh, kw, stride, pad, ptr(wg), ptr(bias), ptr(out), Cout, kpad, epilogue, ptr(gamma),
                                stream_of(x)), "mst_conv_gemm")
    return out


def conv_gemm16(x: torch.Tensor, wg: torch.Tensor, bias: Optional[torch.Tensor], kh: int, kw: int, stride: int, pad: int, *,
                epilogue: int = EPI_BIAS, out: Optional[torch.Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """mst_conv_gemm16: convolution of x [n,H,W,Cin] (NHWC bf16 / fp16, Cin % 64 == 0) with wg [Cout, kh*kw*Cin] of the same type as an
    implicit GEMM on 16-bit MFMA operands -> [n*Ho*Wo, Cout] (the operand type, or fp32).  out: the 16-bit residual operand of
    EPI_RESIDUAL_RELU (updated in place)."""
    _dev(x, "conv_gemm16")
    _dev(wg, "conv_gemm16")
    n, H, W, Cin = x.shape
    Cout = wg.shape[0]
    if wg.shape[1] != kh * kw * Cin:
        raise ValueError(f"conv_gemm16: weight [{Cout}, {wg.shape[1]}] does not match kh*kw*Cin = {kh * kw * Cin}")
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    if out is None:
        out = torch.empty((n * Ho * Wo, Cout), dtype=out_dtype or x.dtype, device=x.device)
    _check(load().mst_conv_gemm16(ptr(x), dt_of(x), n, H, W, Cin, kh, kw, stride, pad, ptr(wg), ptr(bias), ptr(out), dt_of(out), Cout, epilogue,
                                  stream_of(x)), "mst_conv_gemm16")
    return out


def conv_dgrad(dz: torch.Tensor, wt: torch.Tensor, k: int, stride: int, pad: int, H: int, W: int) -> torch.Tensor:
    """mst_conv_dgrad: gradient of a convolution's input from dz [n,Ho,Wo,Cout] (fp32 / bf16 / fp16) and the flipped, transposed weight
    wt [Cin, k*k*Cout] (conv_dgrad_weight) -> dx [n,H,W,Cin] fp32."""
    _dev(dz, "conv_dgrad")
    _dev(wt, "conv_dgrad")
    n, Ho, Wo, Cout = dz.shape
    Cin = wt.shape[0]
    if wt.shape[1] != k * k * Cout or wt.dtype != dz.dtype:
        raise ValueError(f"conv_dgrad: weight {tuple(wt.shape)} {wt.dtype} does not match k*k*Cout = {k * k * Cout} of {dz.dtype}")
    dx = torch.empty((n, H, W, Cin), dtype=torch.float32, device=dz.device)
    _check(load().mst_conv_dgrad(ptr(dz), dt_of(dz), n, Ho, Wo, Cout, k, k, stride, pad, ptr(wt), H, W, Cin, ptr(dx), stream_of(dz)), "mst_conv_dgrad")
    return dx


def conv_dgrad_stem(dz: torch.Tensor, wg: torch.Tensor, k: int, stride: int, pad: int, H: int, W: int, Cin: int,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """mst_conv_dgrad_stem: gradient of a thin-input convolution's input (Cin 1, 2 or 3: the ResNet stem) from dz [n,Ho,Wo,Cout] (fp32 /
    bf16 / fp16) and the forward's GEMM weight wg [Cout, k*k*Cin] in (ky, kx, c) order, of dz's type -> dx [n,H,W,Cin] fp32.  Every element
    of `out` is written; no atomics, no workspace."""
    if not isinstance(dz, torch.Tensor) or not isinstance(wg, torch.Tensor):
        raise TypeError("conv_dgrad_stem: dz and wg must be tensors")
    if dz.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError(f"conv_dgrad_stem: dz is {dz.dtype} (fp32, bf16 or fp16)")
    if wg.dtype != dz.dtype:
        raise TypeError(f"conv_dgrad_stem: dz is {dz.dtype}, wg is {wg.dtype}")
    if dz.dim() != 4:
        raise ValueError(f"conv_dgrad_stem: dz must be [n, Ho, Wo, Cout], got {tuple(dz.shape)}")
    n, Ho, Wo, Cout = dz.shape
    if tuple(wg.shape) != (Cout, k * k * Cin) or wg.device != dz.device:
        raise ValueError(f"conv_dgrad_stem: weight {tuple(wg.shape)} on {wg.device} does not match [Cout, k*k*Cin] = [{Cout}, {k * k * Cin}] on {dz.device}")
    if not dz.is_cuda:
        raise ValueError(f"conv_dgrad_stem: tensors must live on a HIP device (got {dz.device}); the MST kernels have no CPU path")
    if not dz.is_contiguous() or not wg.is_contiguous():
        raise ValueError("conv_dgrad_stem: dz and wg must be contiguous")
    if (Ho, Wo) != ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1):
        raise ValueError(f"conv_dgrad_stem: dz {Ho} x {Wo} is not the output of a {H} x {W} input (k {k}, stride {stride}, padding {pad})")
    if out is None:
        out = torch.empty((n, H, W, Cin), dtype=torch.float32, device=dz.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (n, H, W, Cin) or out.device != dz.device:
        raise ValueError(f"conv_dgrad_stem: out must be contiguous fp32 [{n}, {H}, {W}, {Cin}] on dz's device")
    _check(load().mst_conv_dgrad_stem(ptr(dz), dt_of(dz), n, Ho, Wo, Cout, k, k, stride, pad, ptr(wg), H, W, Cin, ptr(out), stream_of(dz)),
           "mst_conv_dgrad_stem")
    return out


def conv_wgrad(dz: torch.Tensor, x: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    """mst_conv_wgrad(16) + mst_colsum: gradient of a convolution's weight from dz [n*Ho*Wo, Cout] and the input x [n,H,W,Cin] (both fp32, or
    both bf16 / fp16; Cin % 64 == 0) -> fp32 [Cout, k*k*Cin] in (ky, kx, c) order.  The pixels are split into enough partial products to fill
    the chip."""
    _dev(dz, "conv_wgrad")
    _dev(x, "conv_wgrad")
    n, H, W, Cin = x.shape
    rows, Cout = dz.shape
    K = k * k * Cin
    lo = dz.dtype != torch.float32
    if x.dtype != dz.dtype:
        raise ValueError(f"conv_wgrad: dz is {dz.dtype}, x is {x.dtype}")
    tile, step = (128, 64) if lo else (64, 16)
    tiles = ((K + tile - 1) // tile) * ((Cout + tile - 1) // tile)
    nsplit = max(1, min(1024, 2048 // tiles, (rows + 255) // 256))
    rps = (-(-rows // nsplit) + step - 1) // step * step
    nsplit = -(-rows // rps)
    part = torch.empty((nsplit, Cout * K), dtype=torch.float32, device=dz.device)
    if lo:
        _check(load().mst_conv_wgrad16(ptr(dz), ptr(x), dt_of(dz), n, H, W, Cin, k, k, stride, pad, Cout, ptr(part), nsplit, rps, stream_of(dz)),
               "mst_conv_wgrad16")
    else:
        _check(load().mst_conv_wgrad(ptr(dz), ptr(x), n, H, W, Cin, k, k, stride, pad, Cout, ptr(part), nsplit, rps, stream_of(dz)), "mst_conv_wgrad")
    if nsplit == 1:
        return part.view(Cout, K)
    return colsum(part, torch.zeros(Cout * K, dtype=torch.float32, device=dz.device)).view(Cout, K)


def conv_dgrad_weight(weight: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """[Cout, Cin, k, k] -> the operand mst_conv_dgrad multiplies by: [Cin, (ky', kx', co)] with both kernel axes flipped."""
    Cout, Cin, k, _ = weight.shape
    return weight.detach().flip(2, 3).permute(1, 2, 3, 0).reshape(Cin, k * k * Cout).to(dtype).contiguous()


def cvt32(x: torch.Tensor) -> torch.Tensor:
    """mst_cvt32: fp32 copy of a 16-bit tensor."""
    _dev(x, "cvt32")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _check(load().mst_cvt32(ptr(x), dt_of(x), x.numel(), ptr(out), stream_of(x)), "mst_cvt32")
    return out


def maxpool_nhwc(x: torch.Tensor) -> torch.Tensor:
    _dev(x, "maxpool_nhwc")
    n, H, W, Cc = x.shape
    y = torch.empty((n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), dtype=x.dtype, device=x.device)
    if x.dtype == torch.float32:
        _check(load().mst_maxpool_nhwc(ptr(x), n, H, W, Cc, ptr(y), stream_of(x)), "mst_maxpool_nhwc")
    else:
        _check(load().mst_maxpool_nhwc16(ptr(x), dt_of(x), n, H, W, Cc, ptr(y), stream_of(x)), "mst_maxpool_nhwc16")
    return y


def avgpool_nhwc(x: torch.Tensor) -> torch.Tensor:
    _dev(x, "avgpool_nhwc")
    n, H, W, Cc = x.shape
    y = torch.empty((n, Cc), dtype=torch.float32, device=x.device)
    if x.dtype != torch.float32:                         # train_storage='16bit' of the ResNet step: the last unit's output in bf16 / fp16
        _check(load().mst_avgpool_nhwc16(ptr(x), dt_of(x), n, H * W, Cc, ptr(y), stream_of(x)), "mst_avgpool_nhwc16")
        return y
    _check(load().mst_avgpool_nhwc(ptr(x), n, H * W, Cc, ptr(y), stream_of(x)), "mst_avgpool_nhwc")
    return y


def batchnorm_train(z: torch.Tensor, bn, residual: Optional[torch.Tensor], relu: bool, momentum: float = 0.1):
    """nn.BatchNorm2d in train mode on z [rows, C] (+ residual of z's type, ReLU): returns (y in z's type, mean, rstd); updates
    bn.running_* in place.  By z's dtype: mst_batchnorm_train / mst_batchnorm_train_ordered (fp32, by the determinism flag) or
    mst_batchnorm_train16 (bf16 / fp16: fixed summation order in both determinism modes)."""
    _dev(z, "batchnorm_train")
    if residual is not None and (residual.dtype != z.dtype or residual.numel() != z.numel()):
        raise ValueError(f"batchnorm_train: residual {tuple(residual.shape)} {residual.dtype} does not match z {tuple(z.shape)} {z.dtype}")
    rows, Cc = z.shape
    dev = z.device
    y = torch.empty_like(z)
    mean = torch.empty(Cc, dtype=torch.float32, device=dev)
    rstd = torch.empty(Cc, dtype=torch.float32, device=dev)
    tail = (ptr(bn.weight.detach()), ptr(bn.bias.detach()), bn.eps, momentum, ptr(residual), 1 if relu else 0, ptr(y), ptr(mean), ptr(rstd),
            ptr(bn.running_mean), ptr(bn.running_var))
    if z.dtype != torch.float32:
        _call_ws("mst_batchnorm_train16", (rows, Cc), z, ptr(z), dt_of(z), rows, Cc, *tail)
    elif deterministic():
        _call_ws("mst_batchnorm_train_ordered", (rows, Cc), z, ptr(z), rows, Cc, *tail)
    else:
        scratch = torch.empty(Cc, dtype=torch.float32, device=dev)
        _check(load().mst_batchnorm_train(ptr(z), rows, Cc, *tail, ptr(scratch), stream_of(z)), "mst_batchnorm_train")
    return y, mean, rstd


def batchnorm_train16(z: torch.Tensor, bn, residual: Optional[torch.Tensor], relu: bool, momentum: float = 0.1):
    """batchnorm_train on a z that must be bf16 / fp16."""
    _is16(z, "batchnorm_train16", "z")
    return batchnorm_train(z, bn, residual, relu, momentum)


def batchnorm_bwd(z: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor, dy: torch.Tensor):
    """fp32 z and a dy the caller has masked already (act_bwd on the saved output): returns (dz, dgamma, dbeta).  batchnorm_bwd16 is the
    16-bit form, which takes the mask from the saved y itself."""
    rows, Cc = z.shape
    dg = torch.zeros(Cc, dtype=torch.float32, device=z.device)
    db = torch.zeros(Cc, dtype=torch.float32, device=z.device)
    dz = torch.empty_like(z)
    if deterministic():
        _call_ws("mst_batchnorm_bwd_ordered", (rows, Cc), z, ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(dy), rows, Cc, ptr(dg), ptr(db),
                 ptr(dz))
        return dz, dg, db
    _check(load().mst_batchnorm_bwd(ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(dy), rows, Cc, ptr(dg), ptr(db), ptr(dz),
                                    stream_of(z)), "mst_batchnorm_bwd")
    return dz, dg, db


def batchnorm_bwd16(z: torch.Tensor, y: Optional[torch.Tensor], mean: torch.Tensor, rstd: torch.Tensor, gamma: torch.Tensor, dy: torch.Tensor,
                    mask_dy_in_place: bool):
    """mst_batchnorm_bwd16 on the saved z (and y: the ReLU mask, None without ReLU) in bf16 / fp16 and the fp32 dy: returns
    (dz in z's type, dgamma, dbeta); mask_dy_in_place also leaves dy * (y > 0) in dy."""
    _is16(z, "batchnorm_bwd16", "z")
    _dev(dy, "batchnorm_bwd16")
    rows, Cc = z.shape
    if dy.dtype != torch.float32 or dy.numel() != z.numel() or (y is not None and (y.dtype != z.dtype or y.numel() != z.numel())):
        raise ValueError(f"batchnorm_bwd16: dy must be fp32 and y {z.dtype}, both of z's shape {tuple(z.shape)}")
    dev = z.device
    dg = torch.empty(Cc, dtype=torch.float32, device=dev)
    db = torch.empty(Cc, dtype=torch.float32, device=dev)
    dz = torch.empty_like(z)
    _call_ws("mst_batchnorm_bwd16", (rows, Cc), z, ptr(z), ptr(y), dt_of(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(dy),
             1 if mask_dy_in_place else 0, rows, Cc, ptr(dg), ptr(db), ptr(dz))
    return dz, dg, db


def col2im_nhwc(dcol: torch.Tensor, dx: torch.Tensor, kh: int, kw: int, stride: int, pad: int):
    """dx [n,H,W,C] += adjoint of im2col_nhwc applied to dcol [n*Ho*Wo, Kpad]."""
    n, H, W, Cc = dx.shape
    if deterministic():
        _check(load().mst_col2im_nhwc_gather(ptr(dcol), n, H, W, Cc, kh, kw, stride, pad, dcol.shape[1], ptr(dx), stream_of(dx)),
               "mst_col2im_nhwc_gather")
        return dx
    _check(load().mst_col2im_nhwc(ptr(dcol), n, H, W, Cc, kh, kw, stride, pad, dcol.shape[1], ptr(dx), stream_of(dx)), "mst_col2im_nhwc")
    return dx


def maxpool_bwd_nhwc(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    n, H, W, Cc = x.shape
    if x.dtype != torch.float32:                         # the pool input saved in bf16 / fp16: the gather form in both determinism modes
        dx = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
        _call_ws("mst_maxpool_bwd_nhwc16", (n, H, W, Cc), x, ptr(x), dt_of(x), ptr(dy), n, H, W, Cc, ptr(dx))
        return dx
    dx = torch.zeros_like(x)
    if deterministic():
        _call_ws("mst_maxpool_bwd_nhwc_gather", (n, H, W, Cc), x, ptr(x), ptr(dy), n, H, W, Cc, ptr(dx))
        return dx
    _check(load().mst_maxpool_bwd_nhwc(ptr(x), ptr(dy), n, H, W, Cc, ptr(dx), stream_of(x)), "mst_maxpool_bwd_nhwc")
    return dx


def avgpool_bwd_nhwc(dy: torch.Tensor, HW: int) -> torch.Tensor:
    n, Cc = dy.shape
    dx = torch.empty((n, HW, Cc), dtype=torch.float32, device=dy.device)
    _check(load().mst_avgpool_bwd_nhwc(ptr(dy), n, HW, Cc, ptr(dx), stream_of(dy)), "mst_avgpool_bwd_nhwc")
    return dx


def gradcampp(act: torch.Tensor, out: torch.Tensor, fc_weight: Optional[torch.Tensor]) -> torch.Tensor:
    """Grad-CAM++ map of the last ReLU output: act [n, HW, C], out [n, O] model output, fc_weight [O, C] or None -> [n, HW]."""
    n, HW, Cc = act.shape
    cam = torch.empty((n, HW), dtype=torch.float32, device=act.device)
    state = torch.empty(2, dtype=torch.float32, device=act.device)
    _check(load().mst_gradcampp(ptr(act), ptr(out), out.shape[1], ptr(fc_weight), n, HW, Cc, ptr(cam), ptr(state), stream_of(act)),
           "mst_gradcampp")
    return cam


class Profiler:
    """Caller-owned per-kernel timer (mst_profiler): attach with ``vit.profiler = prof.handle`` (DinoV2ClassifierSlice.profiler)."""

    def __init__(self):
        self.handle = load().mst_profiler_create()
        if not self.handle:
            raise RuntimeError("mst_profiler_create failed")

    def collect(self):
        """{kind name: (total ms, launches)} since the last collect (waits for the recorded events)."""
        ms = (C.c_double * K_COUNT)()
        cnt = (C.c_int64 * K_COUNT)()
        _check(load().mst_profiler_collect(self.handle, ms, cnt), "mst_profiler_collect")
        lib = load()
        return {lib.mst_kernel_kind_name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(K_COUNT)}

    def close(self):
        if self.handle:
            load().mst_profiler_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
