"""The fp32 HIP training step against float64 autograd through the CPU oracle, at the shapes the workload reaches and the older oracle
comparisons (ViT-S, <= 16 slices, <= 257 tokens) do not: more than 64 slices (a second trip of the 64-lane row loops of the across-slice
softmax, its key-padding mask and RoPE positions >= 64), embedding width 768, 1370 tokens per slice, a 1 x 37 patch grid.

A helper module, not a conftest: the cases, the memoised reference, the comparison and three oracle mutants that each model one kernel
defect.  tests/test_train_parity_cpu.py shows on the CPU that the bar sits 5x above the reference's own fp32 noise and below every mutant's
displacement of every parameter; tests/test_train_parity_gpu.py holds the HIP step to it.

Bar: max |dP_hip - dP_ref| <= 1e-4 * max |dP_ref| + 1e-9 per parameter and for the source gradient.  It comes from the reference alone:
10x the worst fp32-oracle-against-fp64-oracle noise over the five cases (1.1e-5: room for another, equally valid fp32 summation order,
atomics included) and 5x below the smallest displacement of the weakest mutant (one key of 1370 ignored in one block: 5.5e-4 on its
least-moved parameter, slice_fusion.norm.bias)."""
import contextlib
import functools
import math

import torch
import torch.nn.functional as F

from mst import synth

SOURCE = "<source>"
BAR = 1e-4
STATE_SEED, VOLUME_SEED = 41, 141


def _mask66():
    m = torch.zeros(2, 66, dtype=torch.bool)
    m[0, -5:] = True
    m[1, 3] = True
    return m


# measured on the MI355X: worst scaled error over all parameters and the source gradient, atomic step / ordered step (deterministic flag)
#   vitb_126tok        1.29e-5 / 1.29e-5  (encoder.blocks.0.1.norm2.weight)
#   slices66_mask_pos  7.1e-6 / 7.1e-6    (encoder.blocks.0.7.norm1.bias)
#   slices70_rope      8.3e-6 / 8.4e-6    (encoder.blocks.0.0.norm1.weight)
#   tokens1370         6.3e-6 / 6.5e-6    (encoder.blocks.0.0.norm1.weight)
#   grid_1x37          9.7e-6 / 9.7e-6    (encoder.pos_embed)
# (logits within 1.9e-6, loss within 1.8e-6 of the float64 oracle in every case); bar 1e-4 (see the module docstring)
CASES = {  # name -> (model kwargs, source shape, key-padding mask or None)
    "vitb_126tok": (dict(model_size="b"), (2, 1, 3, 70, 56), None),
    "slices66_mask_pos": (dict(use_slice_pos_emb=True), (2, 1, 66, 14, 14), _mask66),
    "slices70_rope": (dict(rotary_positional_encoding="RoPE"), (1, 1, 70, 14, 14), None),
    "tokens1370": (dict(), (1, 1, 1, 518, 518), None),
    "grid_1x37": (dict(), (1, 1, 2, 14, 518), None),
}


def inputs(case):
    """(model kwargs, source [B, 1, D, H, W] fp32, key-padding mask or None, target [B])."""
    kw, shape, mask = CASES[case]
    return kw, synth.synth_volume(shape, VOLUME_SEED), (mask() if mask else None), torch.arange(shape[0]) % 2


def state_dict(kw):
    return synth.synth_state_dict(kw.get("model_size", "s"), STATE_SEED, use_bottleneck=kw.get("use_bottleneck", False),
                                  use_slice_pos_emb=kw.get("use_slice_pos_emb", False),
                                  slice_fusion=kw.get("slice_fusion", "transformer"), rotary=kw.get("rotary_positional_encoding"))


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants: the oracle with one kernel defect each (context managers over oracle.mst_oracle attributes; nothing under oracle/ changes)
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _patched(name, fn):
    from oracle import mst_oracle as O
    orig = getattr(O, name)
    setattr(O, name, fn(orig))
    try:
        yield
    finally:
        setattr(O, name, orig)


def mask_bits_past_64_lost():
    """The key-padding mask of key positions >= 64 (class token = position 0) reads as 'keep': a mask read that stops after the first
    trip of a 64-lane loop.  The same as mask[:, 63:] = False on the [B, D] mask the model is given."""
    def wrap(orig):
        def slice_fusion(sd, x, key_padding_mask=None, *a, **k):
            if key_padding_mask is not None:
                key_padding_mask = key_padding_mask.clone()
                key_padding_mask[:, 64:] = False
            return orig(sd, x, key_padding_mask, *a, **k)
        return slice_fusion
    return _patched("slice_fusion", wrap)


def rope_position_modulo_64():
    """RoPE angles from position % 64: a lane index used where the row index belongs."""
    def wrap(orig):
        def rope_rotate(t, freqs_param):
            L = t.shape[-2]
            ang = (torch.arange(L) % 64).to(t.dtype)[:, None] * freqs_param.to(t.dtype)[None, :]
            ang = ang.repeat_interleave(2, dim=-1)
            tp = t.reshape(*t.shape[:-1], -1, 2)
            rot = torch.stack((-tp[..., 1], tp[..., 0]), dim=-1).reshape(t.shape)
            return t * ang.cos() + rot * ang.sin()
        return rope_rotate
    return _patched("rope_rotate", wrap)


def last_key_lost_in_block_11():
    """The softmax of encoder block 11 ignores the last key (1369 of 1370): a row loop that ends one element early."""
    def wrap(orig):
        def vit_attention(x, sd, p, heads, *a, **k):
            if not p.endswith(".11"):
                return orig(x, sd, p, heads, *a, **k)
            n, N, C = x.shape
            d = C // heads
            qkv = F.linear(x, sd[p + ".attn.qkv.weight"], sd[p + ".attn.qkv.bias"]).reshape(n, N, 3, heads, d).permute(2, 0, 3, 1, 4)
            s = (qkv[0] * (d ** -0.5)) @ qkv[1].transpose(-2, -1)
            probs = torch.cat((s[..., :-1], torch.full_like(s[..., -1:], -math.inf)), dim=-1).softmax(dim=-1)
            out = (probs @ qkv[2]).transpose(1, 2).reshape(n, N, C)
            return F.linear(out, sd[p + ".attn.proj.weight"], sd[p + ".attn.proj.bias"]), probs
        return vit_attention
    return _patched("vit_attention", wrap)


MUTANTS = {  # name -> (context manager, the case it is measured on)
    "mask_bits_past_64_lost": (mask_bits_past_64_lost, "slices66_mask_pos"),
    "rope_position_modulo_64": (rope_position_modulo_64, "slices70_rope"),
    "last_key_lost_in_block_11": (last_key_lost_in_block_11, "tokens1370"),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# reference and comparison
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_grads(case, dtype=torch.float64, mutant=None):
    """torch.autograd through the CPU oracle in `dtype`: (loss, logits, {parameter: gradient or None, "<source>": d source}).
    Memoised per (case, dtype, mutant): callers must leave the tensors unchanged."""
    from oracle import mst_oracle as O
    kw, src, mask, target = inputs(case)
    # (RoPE's frequencies are a buffer-like Parameter with requires_grad = False in the reference, as in test_train_gpu._oracle_grads)
    sd = {k: (v.to(dtype).requires_grad_(not k.endswith("rotary_positional_encoding.freqs")) if v.is_floating_point() else v.clone())
          for k, v in state_dict(kw).items()}
    x = src.to(dtype).requires_grad_()
    with (MUTANTS[mutant][0]() if mutant else contextlib.nullcontext()):
        logits = O.forward(sd, x, model_size=kw.get("model_size", "s"), slice_fusion_type=kw.get("slice_fusion", "transformer"),
                           src_key_padding_mask=mask, rotary=kw.get("rotary_positional_encoding"))["logits"]
        loss = F.cross_entropy(logits, target)
        loss.backward()
    grads = {k: v.grad for k, v in sd.items() if v.is_floating_point()}
    grads[SOURCE] = x.grad
    return float(loss.detach()), logits.detach(), grads


def scaled_errors(got, ref):
    """{name: max |got - ref| / max |ref|} in float64 over every entry the reference has a gradient for.  The two dicts must name the
    same tensors; where the reference has none (mask_token: unused by the forward) `got` must have none or all zeros."""
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    out = {}
    for k, r in ref.items():
        g = got[k]
        if r is None:
            assert g is None or not bool(g.any()), f"{k}: a gradient where the reference has none"
            continue
        assert g is not None, f"no gradient for {k}"
        assert g.shape == r.shape, (k, tuple(g.shape), tuple(r.shape))
        scale = float(r.abs().max())
        assert scale > 0, k
        out[k] = float((g.detach().cpu().double() - r.double()).abs().max()) / scale
    return out


def check(got, ref, bar=BAR):
    """Every entry within max |d| <= bar * max |ref| + 1e-9; returns {name: scaled error}."""
    errs = scaled_errors(got, ref)
    bad = {k: e for k, e in errs.items() if e * float(ref[k].abs().max()) > bar * float(ref[k].abs().max()) + 1e-9}
    assert not bad, f"{len(bad)} of {len(errs)} above {bar:g} * max|ref|: " + ", ".join(
        f"{k} {e:.3e}" for k, e in sorted(bad.items(), key=lambda kv: -kv[1])[:8])
    return errs
