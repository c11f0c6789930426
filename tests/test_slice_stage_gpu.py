"""The across-slice stage (mst_slice_fusion) at every model's width, depth and batch, against the oracle in float64 (``-m gpu``).

Every call goes through the C ABI (hip.FusionWeights, hip.fusion_workspace_bytes, hip.slice_fusion).  The reference is the oracle that
tests/test_oracle_golden.py pins to the reference classes -- oracle.mst_oracle.fuse, and oracle.mst_oracle.slice_fusion(..., heads=16) for
the 16-head widths that fuse's 12 heads do not cover -- run in float64 on the SAME fp32-rounded weights and inputs.

Inputs (one seeded torch.Generator per case): LayerNorm weights 1 + 0.2 n, biases 0.2 n; linear weights n / sqrt(fan-in), biases 0.1 n; RoPE
freqs uniform in (0, 1); cls_token, slice_pos_emb and the slice embeddings n.  Scores are then ~N(0, 1) and a softmax row over 257 keys is far
from one-hot (the median row maximum of the reference is asserted below 0.25 before the kernel runs), so a wrong score for a minor key shows.

Masks are uint8 [B, D] and differ per volume: volume 0 nothing masked, volume 1 its last third, volume 2 everything but slice 0.

Bars.  The stand-in for "an honest fp32 implementation" is the same oracle run in float32 on the same inputs, compared with its float64
run on the CPU.  A quantity's bar is the larger of the op-test bar (features and logits 2e-5, probabilities 5e-6: test_hip_ops.py's
slice-fusion test) and ten times the stand-in's error for that case, written as a constant in CASES.  RoPE costs the stand-in accuracy
through the fp32 sine and cosine of angles up to 316 rad.  Stand-in errors, max abs, masked and unmasked runs (features / logits / probs):

    case             features   logits     probabilities   probability bar
    s                1.28e-06   5.43e-07   7.59e-07        7.59e-06
    b                1.72e-06   -          3.68e-06 RoPE   3.68e-05
    g                1.46e-06   -          1.01e-06        1.01e-05
    g_158            1.65e-06   -          9.82e-07 RoPE   9.82e-06
    g_159            1.57e-06   8.99e-07   1.55e-06 RoPE   1.55e-05
    g_316            1.74e-06   -          1.60e-06 RoPE   1.60e-05
    r18              1.60e-06   4.68e-07   3.52e-06 RoPE   3.52e-05
    r50              1.26e-06   -          4.91e-07        5e-06
    short_g          1.85e-06   -          2.87e-07        5e-06
    short_r50        1.13e-06   -          2.97e-07        5e-06
    bottleneck_pos   1.55e-06   5.26e-07   5.14e-07        5.14e-06
    average          3.32e-08   -          -
    linear           0          4.57e-07   -
  Ten times the features and logits columns stays below 2e-5 everywhere, so those two bars are the op-test bar in every case.

Measured on the MI355X, max abs error over bar (worst of the masked and the unmasked call; features / logits / probabilities):

    s 0.09 0.04 0.09 | b 0.10 - 0.11 | g 0.19 - 0.13 | g_158 0.12 - 0.11 | g_159 0.12 0.08 0.11 | g_316 0.12 - 0.10 | r18 0.11 0.08 0.10
    r50 0.17 - 0.18 | short_g 0.27 - 0.18 | short_r50 0.28 - 0.26 | bottleneck_pos 0.07 0.03 0.10 | average 0.01 - - | linear 0.00 0.22 -
  (absolute: features at most 5.5e-6, probabilities at most 3.9e-6, the latter with RoPE.)  The median row maximum of the float64
  reference is 0.04 to 0.07 in every case of 8 tokens or more.
"""
import dataclasses
import math
import zlib
from typing import Optional

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FEAT_BAR, PROB_BAR = 2e-5, 5e-6         # tests/test_hip_ops.py::test_slice_fusion_matches_reference_layer_fixture
LDS_MAX = 160 * 1024                    # bytes of LDS a workgroup may hold on gfx950


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    emb: int
    heads: int
    B: int
    D: int
    rotary: Optional[str] = None        # None | "RoPE"
    mask: Optional[str] = None          # None | "volumes" (the per-volume pattern above) | "last" (the last slice of every volume)
    emb_in: int = 0                     # != 0: a bottleneck emb_in -> emb
    pos: bool = False                   # slice_pos_emb
    out_ch: int = 0
    fusion: str = "transformer"
    bars: tuple = (FEAT_BAR, FEAT_BAR, PROB_BAR)   # features, logits, probabilities


# What the cases enter (csrc/k_slice.hip, k_layernorm.hip).  LDS of the attention: (2 L hd + L) * 4 bytes, L = D + 1.
#   s               hd 32, 65.3 KiB of LDS (the opt-in above 64 KiB), a second trip of the 256-query loop (L = 257)
#   b               slice_attn_kernel<64>, 129.5 KiB
#   g               <128> at L = 257: past what K and V fill in LDS, the V-from-global form; layernorm_kernel<16>
#   g_158, g_159    the last length with K and V in LDS (159.6 KiB) and the first without
#   g_316           L = 317, the last length the V-from-global form takes (159.7 KiB of K and mask)
#   r18             ResNet-18/34 width, 16 heads of 32
#   r50             bottleneck-ResNet width: <128> with 16 heads, layernorm_kernel<16> at its widest, in_proj 6144 x 2048
#   short_*         L = 2 and L = 3
#   bottleneck_pos  bottleneck_w with emb_in != emb, all 256 rows of slice_pos_emb
#   average, linear mean_slices_kernel; rows_copy_kernel with F = D * emb and the head over F columns
# out_ch = 2 adds head_w and the logits.  bars: max(op-test bar, 10 x stand-in) per case, from the table in the module docstring
CASES = [
    Case("s", 384, 12, 3, 256, mask="volumes", out_ch=2, bars=(FEAT_BAR, FEAT_BAR, 7.59e-6)),
    Case("b", 768, 12, 3, 256, "RoPE", "volumes", bars=(FEAT_BAR, FEAT_BAR, 3.68e-5)),
    Case("g", 1536, 12, 3, 256, mask="volumes", bars=(FEAT_BAR, FEAT_BAR, 1.01e-5)),
    Case("g_158", 1536, 12, 2, 158, "RoPE", bars=(FEAT_BAR, FEAT_BAR, 9.82e-6)),
    Case("g_159", 1536, 12, 2, 159, "RoPE", "volumes", out_ch=2, bars=(FEAT_BAR, FEAT_BAR, 1.55e-5)),
    Case("g_316", 1536, 12, 2, 316, "RoPE", "volumes", bars=(FEAT_BAR, FEAT_BAR, 1.60e-5)),
    Case("r18", 512, 16, 3, 256, "RoPE", "volumes", out_ch=2, bars=(FEAT_BAR, FEAT_BAR, 3.52e-5)),
    Case("r50", 2048, 16, 2, 256, mask="volumes"),
    Case("short_g", 1536, 12, 4, 1),
    Case("short_r50", 2048, 16, 1, 2, mask="last"),
    Case("bottleneck_pos", 384, 12, 2, 256, mask="volumes", emb_in=1536, pos=True, out_ch=2, bars=(FEAT_BAR, FEAT_BAR, 5.14e-6)),
    Case("average", 1536, 0, 3, 200, fusion="average"),
    Case("linear", 384, 0, 2, 32, out_ch=2, fusion="linear"),
]


def make_inputs(c: Case):
    """(sd with the oracle's keys, emb [B*D, emb_in], mask uint8 [B, D] or None): fp32 tensors on the CPU."""
    gen = torch.Generator().manual_seed(zlib.crc32(c.name.encode()))
    n = lambda *shape: torch.randn(*shape, generator=gen)
    E, Ein = c.emb, c.emb_in or c.emb
    sd = {}

    def linear(key, out, inp, bias_key=None):
        sd[key] = n(out, inp) / math.sqrt(inp)
        sd[bias_key or key.replace("weight", "bias")] = 0.1 * n(out)

    def norm(key):
        sd[key + ".weight"], sd[key + ".bias"] = 1 + 0.2 * n(E), 0.2 * n(E)

    if c.emb_in:
        linear("bottleneck.weight", E, Ein)
    if c.pos:
        sd["slice_pos_emb.weight"] = n(256, E)
    if c.fusion == "transformer":
        p = "slice_fusion.layers.0."
        sd["cls_token"] = n(1, 1, E)
        norm(p + "norm1")
        linear(p + "self_attn.in_proj_weight", 3 * E, E, p + "self_attn.in_proj_bias")
        linear(p + "self_attn.out_proj.weight", E, E)
        norm(p + "norm2")
        linear(p + "linear1.weight", E, E)
        linear(p + "linear2.weight", E, E)
        norm("slice_fusion.norm")
        if c.rotary:
            sd[p + "self_attn.rotary_positional_encoding.freqs"] = torch.rand(E // c.heads // 2, generator=gen).clamp_(1e-3, 1 - 1e-3)
    if c.out_ch:
        linear("linear.weight", c.out_ch, c.D * E if c.fusion == "linear" else E)
    emb = n(c.B * c.D, Ein)
    mask = None
    if c.mask == "volumes":
        mask = torch.zeros(c.B, c.D, dtype=torch.uint8)
        mask[1, c.D - c.D // 3:] = 1
        if c.B > 2:
            mask[2, 1:] = 1
    elif c.mask == "last":
        mask = torch.zeros(c.B, c.D, dtype=torch.uint8)
        mask[:, -1] = 1
    return sd, emb, mask


def reference(c: Case, sd, emb, mask, dt):
    """The oracle in dtype dt: (features [B, F], logits [B, out_ch] or None, probabilities [B, heads, L, L] or None)."""
    from oracle import mst_oracle as O
    sd = {k: v.to(dt) for k, v in sd.items()}
    emb = emb.to(dt)
    m = None if mask is None else mask.bool()
    with torch.no_grad():
        if c.fusion != "transformer" or c.heads == O.SLICE_HEADS:
            out = O.fuse(sd, emb, c.B, c.D, slice_fusion_type=c.fusion, src_key_padding_mask=m, rotary=c.rotary)
            return out["features"], out.get("logits"), out["slice_map"]
        # O.fuse fixes 12 heads.  The 16-head widths (ResNetSliceTrans) have neither bottleneck nor slice_pos_emb: give the layer the
        # CLS row and the unmasked CLS column as O.fuse does, and call it with its heads
        assert not c.emb_in and not c.pos
        x = torch.cat([sd["cls_token"].repeat(c.B, 1, 1), emb.reshape(c.B, c.D, -1)], dim=1)
        if m is not None:
            m = torch.cat([torch.zeros(c.B, 1, dtype=torch.bool), m], dim=1)
        y, probs = O.slice_fusion(sd, x, m, c.rotary, heads=c.heads)
        feat = y[:, 0]
        return feat, (F.linear(feat, sd["linear.weight"], sd["linear.bias"]) if c.out_ch else None), probs


@pytest.fixture(scope="module")
def hip():
    from mst import hip as h
    h.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return h


def fusion_weights(hip, c: Case, sd):
    """hip.FusionWeights over device copies of sd; returns (fw, the tensors it points to)."""
    dev = {k: v.contiguous().cuda() for k, v in sd.items()}
    fw = hip.FusionWeights()
    fw.emb_in, fw.emb, fw.out_ch, fw.num_heads = c.emb_in or c.emb, c.emb, c.out_ch, c.heads
    fw.fusion_type = {"transformer": hip.FUSION_TRANSFORMER, "linear": hip.FUSION_LINEAR, "average": hip.FUSION_AVERAGE}[c.fusion]
    p = "slice_fusion.layers.0."
    names = {"bottleneck_w": "bottleneck.weight", "bottleneck_b": "bottleneck.bias", "slice_pos_emb": "slice_pos_emb.weight",
             "cls_token": "cls_token", "ln1_w": p + "norm1.weight", "ln1_b": p + "norm1.bias",
             "in_proj_w": p + "self_attn.in_proj_weight", "in_proj_b": p + "self_attn.in_proj_bias",
             "out_proj_w": p + "self_attn.out_proj.weight", "out_proj_b": p + "self_attn.out_proj.bias",
             "ln2_w": p + "norm2.weight", "ln2_b": p + "norm2.bias", "lin1_w": p + "linear1.weight", "lin1_b": p + "linear1.bias",
             "lin2_w": p + "linear2.weight", "lin2_b": p + "linear2.bias", "norm_w": "slice_fusion.norm.weight",
             "norm_b": "slice_fusion.norm.bias", "rope_freqs": p + "self_attn.rotary_positional_encoding.freqs",
             "head_w": "linear.weight", "head_b": "linear.bias"}
    for field, key in names.items():
        if key in dev:
            setattr(fw, field, dev[key].data_ptr())
    return fw, dev


def run_stage(hip, c: Case, fw, emb_dev, mask):
    """One hip.slice_fusion call into NaN-filled outputs: (features, logits or None, probabilities or None) on the CPU."""
    L = c.D + 1
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    feat = nan(c.B, c.D * c.emb if c.fusion == "linear" else c.emb)
    logits = nan(c.B, c.out_ch) if c.out_ch else None
    probs = nan(c.B, c.heads, L, L) if c.fusion == "transformer" else None
    ws = torch.empty(hip.fusion_workspace_bytes(fw, c.B, c.D), dtype=torch.uint8, device="cuda")
    hip.slice_fusion(fw, emb_dev, c.B, c.D, None if mask is None else mask.cuda(), feat, logits, probs, ws)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (feat, logits, probs))


def median_row_max(probs):
    return float(probs.max(dim=-1).values.flatten().median())


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_slice_stage_matches_float64_oracle(hip, c):
    sd, emb, mask = make_inputs(c)
    L = c.D + 1
    refs = {"plain": reference(c, sd, emb, None, torch.float64)}
    if mask is not None:
        refs["masked"] = reference(c, sd, emb, mask, torch.float64)
    if c.fusion == "transformer":
        # the softmax rows must not be one-hot.  A row of L keys has a maximum of at least 1 / L, so the figure can hold from L = 8 on;
        # the two- and three-token cases are there for the indexing at L = 2, 3
        for tag, (_, _, rp) in refs.items():
            med = median_row_max(rp)
            print(f"slice stage {c.name} {tag}: reference median row maximum {med:.3f}")
            assert L < 8 or med < 0.25, (tag, med)
    fw, dev = fusion_weights(hip, c, sd)
    emb_dev = emb.cuda()
    worst = [0.0, 0.0, 0.0]
    for tag, ref in refs.items():
        m = mask if tag == "masked" else None
        got = run_stage(hip, c, fw, emb_dev, m)
        errs = []
        for i, (g, r) in enumerate(zip(got, ref)):
            assert (g is None) == (r is None)
            if g is None:
                errs.append(0.0)
                continue
            assert g.shape == r.shape and not torch.isnan(g).any(), (tag, i)          # every element written
            errs.append(float((g.double() - r).abs().max()))
            worst[i] = max(worst[i], errs[i] / c.bars[i])
        print(f"slice stage {c.name} {tag}: max abs error features {errs[0]:.2e} logits {errs[1]:.2e} probabilities {errs[2]:.2e}")
        probs = got[2]
        if probs is not None:
            assert float((probs.double().sum(-1) - 1).abs().max()) < 1e-5
            if m is not None:
                for b in range(c.B):
                    cols = 1 + torch.nonzero(m[b]).flatten()                          # column 0 is the CLS token
                    assert torch.equal(probs[b][:, :, cols], torch.zeros(c.heads, L, len(cols))), b
        for i, what in enumerate(("features", "logits", "probabilities")):
            assert errs[i] < c.bars[i], (tag, what, errs[i], c.bars[i])
    print(f"slice stage {c.name}: error / bar, features {worst[0]:.2f} logits {worst[1]:.2f} probabilities {worst[2]:.2f}")
    del dev


def _lds_fits(L, hd):
    """launch_slice_attn's rule (csrc/k_slice.hip): K, V and the additive mask in LDS, (2 L hd + L) floats; head_dim 128 may keep K and
    the mask alone, (L hd + L) floats, and read V from global memory."""
    return (2 * L * hd + L) * 4 <= LDS_MAX or (hd == 128 and (L * hd + L) * 4 <= LDS_MAX)


def test_extent_of_the_lds_limit(hip):
    """head_dim 128 runs at L = 257, the length slice_pos_emb allows; the first length the rule above does not fit is refused with a message
    that names L and head_dim, before anything is launched that could not run.  The same for head_dim 64, which has the LDS form only."""
    lib = hip.load()
    assert _lds_fits(257, 128) and _lds_fits(257, 64)
    for E, hd, runs in ((1536, 128, 257), (768, 64, None)):
        c = Case("extent", E, E // hd, 1, 1)
        sd, _, _ = make_inputs(c)
        fw, dev = fusion_weights(hip, c, sd)
        L_max = max(L for L in range(2, 1024) if _lds_fits(L, hd))
        # K alone at head_dim 128 takes what K and V take at 64: L (128 + 1) floats either way
        assert L_max == LDS_MAX // (4 * 129) == 317 and not _lds_fits(L_max + 1, hd)
        for L in filter(None, (runs, L_max + 1)):
            D = L - 1
            emb = torch.randn(D, E, generator=torch.Generator().manual_seed(L)).cuda()
            feat = torch.full((1, E), float("nan"), device="cuda")
            ws = torch.empty(hip.fusion_workspace_bytes(fw, 1, D), dtype=torch.uint8, device="cuda")
            rc = lib.mst_slice_fusion(hip.C.byref(fw), emb.data_ptr(), 1, D, None, feat.data_ptr(), None, None, ws.data_ptr(), ws.numel(),
                                      hip.stream_of(emb))
            torch.cuda.synchronize()
            if L <= L_max:
                assert rc == 0, hip.last_error()
                assert not torch.isnan(feat).any()
            else:
                assert rc != 0
                assert f"L={L} " in hip.last_error() and f"head_dim={hd} " in hip.last_error(), hip.last_error()
                assert torch.isnan(feat).all()                                         # refused, not answered
        del dev
