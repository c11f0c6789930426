"""What the folded test-time-augmentation tests share (tests/test_tta_folded_cpu.py, tests/test_tta_folded_gpu.py): the bars, the two
order-sensitive models with their input, the CPU oracle's answer for them (computed once), and a restatement of the folded algorithm
on the oracle's own pieces whose two switches also produce the two WRONG readings the tests must be able to tell from the right one.

Bars: the project's own TOL table (tests/test_model_gpu.py), logits / pred absolute and volumes relative-L2:

    mode    pred / logits (abs)    volumes (rel-L2)
    fp32    1e-4                   1e-3
    fp16    5e-3                   1e-2
"""
from functools import lru_cache

import torch

from mst import synth
from oracle import mst_oracle as O

TOL = {"fp32": (1e-4, 1e-3), "fp16": (5e-3, 1e-2)}        # tests/test_model_gpu.py TOL: (logits abs, maps rel)

# Models whose slice transformer sees the slice ORDER (a learned position per slice; rotary positions): without one of them the
# transformer is permutation-equivariant and a wrong depth reversal would go unnoticed.
ORDER_CASES = {
    "bottleneck_pos": dict(use_bottleneck=True, use_slice_pos_emb=True),
    "rope": dict(rotary_positional_encoding="RoPE"),
}
ORDER_SHAPE = (1, 1, 5, 56, 56)                            # odd D: the reversal has a centre
ORDER_SEED = 21
TTA_MASKS = (0, 1, 2, 4, 3, 5, 6, 7)                       # (), (2,), (3,), (4,), (2,3), (2,4), (3,4), (2,3,4): bit 0 D, bit 1 H, bit 2 W


def state_dict(kw, seed):
    return synth.synth_state_dict(kw.get("model_size", "s"), seed, use_bottleneck=kw.get("use_bottleneck", False),
                                  use_slice_pos_emb=kw.get("use_slice_pos_emb", False),
                                  slice_fusion=kw.get("slice_fusion", "transformer"), rotary=kw.get("rotary_positional_encoding"))


def build(kw, seed, mode, **extra):
    from mst.models import DinoV2ClassifierSlice
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode, **kw, **extra)
    model.load_state_dict(state_dict(kw, seed), strict=True)
    return model.cuda().eval()


def order_inputs():
    """(source, mask): only slice 1 of 5 is padding, which a depth flip moves to slice 3."""
    src = synth.synth_volume(ORDER_SHAPE, ORDER_SEED + 100)
    mask = torch.zeros(1, ORDER_SHAPE[2], dtype=torch.bool)
    mask[0, 1] = True
    return src, mask


@lru_cache(maxsize=None)
def oracle_run_pred(name):
    """oracle.run_pred(use_tta=True) on an ORDER_CASES model: the script's eight forwards, restated on the CPU."""
    kw = ORDER_CASES[name]
    src, mask = order_inputs()
    with torch.no_grad():
        return O.run_pred(state_dict(kw, ORDER_SEED), src, use_softmax=True, use_tta=True, src_key_padding_mask=mask,
                          rotary=kw.get("rotary_positional_encoding"))


def restated_run_pred(name, *, flip_mask_with_d=False, reverse_embeddings=True):
    """The folded algorithm on the oracle's pieces: four encoder passes (the in-plane flips), eight fusions.  The defaults are the
    right reading; flip_mask_with_d=True mirrors the padding mask together with D (the script does not: main_predict.py:149), and
    reverse_embeddings=False feeds the depth-flipped variants the slices in their original order."""
    kw = ORDER_CASES[name]
    sd, rotary = state_dict(kw, ORDER_SEED), kw.get("rotary_positional_encoding")
    src, mask = order_inputs()
    _, _, D, H, W = src.shape
    pred = low = ws = None
    with torch.no_grad():
        encoded = []
        for f in range(4):
            dims = tuple(a for a, bit in ((1, 1), (2, 2)) if f & bit)
            emb, maps = O.vit_encode(sd, torch.flip(src[0, 0], dims) if dims else src[0, 0], "s", "cls")
            plane = O.plane_attention(maps[-1]).mean(dim=1)                      # [D, Np]
            g = int(plane.shape[-1] ** 0.5)
            plane = plane[:, :g * g].reshape(D, g, g)
            encoded.append((emb, torch.flip(plane, dims) if dims else plane))   # the in-plane flip undone
        for m in TTA_MASKS:
            (emb, plane), r = encoded[m >> 1], m & 1
            out = O.fuse(sd, emb.flip(0) if (r and reverse_embeddings) else emb, 1, D,
                         src_key_padding_mask=mask.flip(1) if (r and flip_mask_with_d) else mask, rotary=rotary)
            sa = O.slice_attention(out["slice_map"]).reshape(D)
            sa = sa.flip(0) if r else sa                                         # back to the volume's own slice order
            p = out["logits"].softmax(-1)
            pred = p if pred is None else pred + p
            low = plane * sa[:, None, None] if low is None else low + plane * sa[:, None, None]
            ws = sa if ws is None else ws + sa
    weight = O.trilinear_upsample((low / 8)[None, None], (D, H, W))
    return pred / 8, weight, (ws / 8).reshape(1, 1, D, 1, 1) * torch.ones_like(src)
