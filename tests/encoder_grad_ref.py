"""Gradients through the encoder API (``model.encoder.forward`` / ``forward_features`` / ``get_intermediate_layers`` with
``encoder_grad=True``) against float64 torch.autograd through the CPU restatement tests/encoder_ref.py::Restated.

A helper module, not a conftest: the cases, the loss, the memoised reference, the device run and three mutants of the reference that each
model one defect.  tests/test_encoder_grad_cpu.py shows on the CPU that the bar sits 5x above the reference's own fp32 noise and 5x below
every mutant's displacement of the parameter it aims at; tests/test_encoder_grad_gpu.py holds the HIP path to it.

Loss of a case: a fixed linear functional of EVERY output of EVERY call of the case, sum_k (c_k * out_k).sum() / out_k.numel() with c_k standard
normals from mst.synth (seed LOSS_SEED + k): every row and every tap pulls differently, and the same loss is built on the device outputs.

Bar: train_parity.BAR = 1e-4 (max |g - ref| <= 1e-4 * max |ref| + 1e-9 per parameter and for x.grad), kept because it sits in the sandwich
measured on the CPU (fp32 restatement against the float64 one; mutants on rgb_56x70):
  noise, worst parameter per case:  rgb_56x70 8.2e-6  rgb_70x84 7.4e-6  grey_28x42 5.9e-6  b_28x42 4.9e-6
                                    reg_56x56 1.35e-5  swiglu_28x28 1.07e-5  tap3_only 3.4e-6  wgrad_splits 6.7e-6
  (all at or below a fifth of the bar, 2e-5)
  mutant displacement of the aimed parameter:  middle_tap_dropped 4.4e-1 (blocks.0.5.mlp.fc2.bias; 79 of 151 tensors move by 5 bars or more)
      final_norm_cls_rows_only 9.8e-2 (norm.weight; all 151)   dw_channels_swapped 1.65 (patch_embed.proj.weight; that tensor alone)
  (all at or above five times the bar, 5e-4)

wgrad_splits: mst_patch_embed_rgb_wgrad splits the patch rows 256 at a time (mst.hip.rgb_wgrad_split_rows; more per split only beyond 4096
rows).  [2, 3, 140, 196] is 2 x 140 = 280 patch rows: two partials, the second ragged (24 rows: one whole 16-row K-step and half of one),
and the seam of the two images (row 140) inside the first.

Measured on the MI355X (worst scaled error over all parameters and x.grad, fp32, atomic reductions; the tensor it falls on):
  rgb_56x70 7.5e-6 (blocks.0.1.norm1.weight)   rgb_70x84 7.9e-6 (blocks.0.2.norm1.weight)   grey_28x42 9.0e-6 (blocks.0.0.norm1.weight)
  b_28x42 9.4e-6 (blocks.0.0.attn.qkv.bias)    reg_56x56 1.09e-5 (blocks.0.norm1.weight)    swiglu_28x28 1.71e-5 (blocks.0.2.attn.qkv.weight)
  tap3_only 4.0e-6 (blocks.0.1.norm2.weight)   wgrad_splits 7.4e-6 (patch_embed.proj.weight);   x.grad between 3.0e-6 and 1.08e-5.
Op level (tests/test_encoder_grad_gpu.py): forward <= 6.6e-7, input gradient <= 1.0e-6 (bar 1e-5), weight gradient <= 6.6e-7 (bar 1e-4).
Mixed modes at [2, 3, 56, 224] against the fp32 run, worst tensor / all together: fp16 3.7e-3 / 3.2e-3 (bars 1e-2 / 8e-3), bf16 + flash + 16bit
4.0e-2 / 3.3e-2 (bars 1.3e-1 / 7e-2); x.grad 3.6e-3 and 3.9e-2.
"""
import contextlib
import functools

import torch

import encoder_ref as ER
from mst import synth
from train_parity import BAR, check, scaled_errors  # noqa: F401  (the comparison of the training-step parity tests)

SOURCE = "<x>"
STATE_SEED, IMAGE_SEED, LOSS_SEED = 41, 241, 9000

FF = ("forward_features", {})
CASES = {  # name -> (model kind, x shape, calls)
    "rgb_56x70": ("s", (2, 3, 56, 70), (FF, ("get_intermediate_layers", dict(n=[0, 5, 11], reshape=True, return_class_token=True)),
                                         ("get_intermediate_layers", dict(n=[3], norm=False)), ("forward", {}))),
    "rgb_70x84": ("s", (3, 3, 70, 84), (FF,)),
    "grey_28x42": ("s", (2, 1, 28, 42), (FF,)),
    "b_28x42": ("b", (1, 3, 28, 42), (FF,)),
    "reg_56x56": ("reg", (2, 3, 56, 56), (FF,)),
    "swiglu_28x28": ("swiglu", (2, 3, 28, 28), (FF,)),
    "tap3_only": ("s", (2, 3, 28, 42), (("get_intermediate_layers", dict(n=[3], norm=False)),)),
    "wgrad_splits": ("s", (2, 3, 140, 196), (FF,)),
}
MODELS = {  # kind -> (constructor keywords, synth_state_dict keywords, model_size, heads)
    "s": ({}, {}, "s", 6),
    "b": (dict(model_size="b"), {}, "b", 12),
    "reg": (dict(use_registers=True), dict(img_size=56, layerscale=True, chunked=False, num_register_tokens=4), "s", 6),
    "swiglu": (dict(ffn_layer="swiglufused"), dict(ffn_layer="swiglufused"), "s", 6),
}
MUTANTS = {  # name -> the parameter it aims at (measured on rgb_56x70)
    "middle_tap_dropped": "encoder.blocks.0.5.mlp.fc2.bias",
    "final_norm_cls_rows_only": "encoder.norm.weight",
    "dw_channels_swapped": "encoder.patch_embed.proj.weight",
}


def state_dict(case):
    kind = CASES[case][0]
    return synth.synth_state_dict(MODELS[kind][2], STATE_SEED, **MODELS[kind][1])


def image(case):
    shape = CASES[case][1]
    if shape[1] == 3:
        return ER.rgb_image(shape, IMAGE_SEED)
    return synth.synth_volume((1, 1, shape[0], shape[2], shape[3]), IMAGE_SEED)[0, 0][:, None].contiguous()


def build_model(case, mode="fp32", encoder_grad=True, **extra):
    """The case's DinoV2ClassifierSlice on the device, its state loaded."""
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    kind = CASES[case][0]
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode, encoder_grad=encoder_grad, **MODELS[kind][0], **extra)
    if kind == "reg":
        model.encoder = _ViT(384, 12, 6, img_size=56, num_register_tokens=4, layerscale=1.0, chunked=False)
    model.load_state_dict(state_dict(case), strict=True)
    return model.cuda().eval()


def outputs(enc, x, calls, mutant=None):
    """[(name, tensor)] of every non-empty output of every call, in call order.  enc: model.encoder (x on the device) or an ER.Restated."""
    dev = isinstance(enc, torch.nn.Module)
    out = []
    for i, (method, kw) in enumerate(calls):
        res = getattr(enc, method)(x, **kw) if dev else getattr(enc, method)(**kw)
        if method == "forward":
            out.append((f"{i}.forward", res))
        elif method == "forward_features":
            if mutant == "final_norm_cls_rows_only":      # the patch (and register) rows' gradient at the final norm is lost
                res = {k: (v.detach() if k in ("x_norm_patchtokens", "x_norm_regtokens") else v) for k, v in res.items()}
            out += [(f"{i}.ff.{k}", res[k]) for k in ("x_norm_clstoken", "x_norm_regtokens", "x_norm_patchtokens", "x_prenorm")]
        else:
            flat = [t for r in res for t in (r if isinstance(r, tuple) else (r,))]
            per = len(flat) // len(res)
            for j, t in enumerate(flat):
                if mutant == "middle_tap_dropped" and len(res) >= 3 and j // per == len(res) // 2:
                    t = t.detach()                         # the gradient of a middle tap never joins d x
                out.append((f"{i}.il.{j}", t))
    return [(k, t) for k, t in out if t.numel()]


def loss_of(outs):
    total = 0.0
    for k, (_, t) in enumerate(outs):
        c = torch.from_numpy(synth.hash_normal(tuple(t.shape), LOSS_SEED + k)).to(device=t.device, dtype=t.dtype)
        total = total + (c * t).sum() / t.numel()
    return total


@functools.lru_cache(maxsize=None)
def ref_grads(case, dtype=torch.float64, mutant=None):
    """torch.autograd through the restatement in `dtype`: (loss, [(name, output)], {"encoder.<parameter>": gradient or None, "<x>": d x}).
    Memoised: callers leave the tensors unchanged."""
    kind, _, calls = CASES[case]
    sd = {k: (v.to(dtype).requires_grad_(k.startswith("encoder.")) if v.is_floating_point() else v.clone()) for k, v in state_dict(case).items()}
    x = image(case).to(dtype).requires_grad_()
    depth = 1 + max(int(k.split(".")[-3]) for k in sd if k.endswith(".norm1.weight"))
    ref = ER.Restated(sd, x, depth, MODELS[kind][3], dtype=dtype)
    outs = outputs(ref, None, calls, mutant)
    loss = loss_of(outs)
    loss.backward()
    grads = {k: v.grad for k, v in sd.items() if k.startswith("encoder.") and v.is_floating_point()}
    if mutant == "dw_channels_swapped":
        grads["encoder.patch_embed.proj.weight"] = grads["encoder.patch_embed.proj.weight"][:, [0, 2, 1]].contiguous()
    grads[SOURCE] = x.grad
    return float(loss.detach()), [(k, t.detach()) for k, t in outs], grads


def device_grads(model, case, x=None):
    """One forward + backward of the case's calls and loss on the device: (loss, [(name, output)], gradients named as `ref_grads` names them)."""
    x = (image(case) if x is None else x).cuda().requires_grad_()
    for p in model.parameters():
        p.grad = None
    outs = outputs(model.encoder, x, CASES[case][2])
    loss = loss_of(outs)
    loss.backward()
    grads = {"encoder." + k: p.grad for k, p in model.encoder.named_parameters()}
    grads[SOURCE] = x.grad
    return float(loss.detach()), [(k, t.detach()) for k, t in outs], grads


@contextlib.contextmanager
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
