"""Which pipeline a forward of DinoV2ClassifierSlice takes through mst_vit_encode, pinned by the per-kind launch counts of the
caller-owned profiler (mst_profiler: one record per RUNK launch), for ViT-S (depth 12) with seed-0 synth weights.

The encoder picks its kernels from what it can observe: compute dtype, embed_dim, the token count of the whole call (fused
pipeline from MST_FUSED_MIN_TOKENS = 12,288 tokens up), which packed weights the caller filled (the Python side fills all of
them for 16-bit ViT-S), fp8_linear and prune_last_block.  Two shapes straddle the crossover: 1 x 48 x 224^2 = 12,336 tokens and
1 x 4 x 112^2 = 260 tokens.  Every configuration is also compared with the CPU oracle at the logits tolerances of
tests/test_model_gpu.py and smoke() (fp32 1e-4, fp16 5e-3, bf16 3e-2).  Those files set no logits bar for fp8 at an arbitrary
shape (two logits behind the across-slice transformer are a noisy statistic of e4m3 rounding), so the fp8 rows take the bar
tests/test_fp8_gpu.py::_noise_check applies to every shape: the embeddings lie within 1.5x the fp8 oracle's own quantisation
noise of both the exact and the fp8 oracle.  The calibrated run uses the table recorded on the same volume, which holds the
scales the dynamic run finds.
"""
import functools

import pytest
import torch

from conftest import rel_l2
from mst import synth

pytestmark = pytest.mark.gpu

DEPTH = 12
BIG, SMALL = (1, 1, 48, 224, 224), (1, 1, 4, 112, 112)
TOL = {"fp32": 1e-4, "fp16": 5e-3, "bf16": 3e-2}
KINDS = ("patch_embed", "layernorm", "gemm_qkv", "attention", "gemm_proj", "gemm_fc1", "gemm_fc2", "cls_probs", "mlp_fused",
         "block_fused")
UNFUSED = dict(patch_embed=1, layernorm=2 * DEPTH, gemm_qkv=DEPTH, attention=DEPTH, gemm_proj=DEPTH, gemm_fc1=DEPTH, gemm_fc2=DEPTH)
FUSED = dict(patch_embed=1, gemm_qkv=DEPTH, attention=DEPTH, block_fused=DEPTH)
# prune_last_block: the last block runs for the CLS rows on the unfused kernels (its attention launch counts as 'attention')
PRUNED = dict(patch_embed=1, gemm_qkv=DEPTH, attention=DEPTH, block_fused=DEPTH - 1, gemm_proj=1, layernorm=1, gemm_fc1=1, gemm_fc2=1)


def _plus(counts, **more):
    return {**counts, **more}


@functools.lru_cache(maxsize=None)
def _volume(shape):
    return synth.synth_volume(shape, 123)


@functools.lru_cache(maxsize=None)
def _oracle(shape, linear=None):
    from oracle import mst_oracle as O
    kw = {} if linear is None else dict(linear=linear)
    with torch.no_grad():
        return O.forward(synth.synth_state_dict("s", 0), _volume(shape), keep="cls", **kw)


def _model(mode, **kw):
    from mst.models import DinoV2ClassifierSlice
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode, **kw)
    model.load_state_dict(synth.synth_state_dict("s", 0), strict=True)
    return model.cuda().eval()


def _profiled_forward(model, shape, save_attn=False):
    """One no_grad forward with the profiler attached -> (logits on the CPU, {kind: launches})."""
    from mst import hip
    model.profiler = hip.Profiler()
    try:
        with torch.no_grad():
            logits = model(_volume(shape), save_attn=save_attn).cpu()
        counts = {k: n for k, (_, n) in model.profiler.collect().items()}
    finally:
        model.profiler.close()
        model.profiler = None
    assert set(counts) == set(KINDS)
    return logits, counts


def _expect(counts, want):
    assert counts == {k: want.get(k, 0) for k in KINDS}


CASES = {
    "bf16_big": ("bf16", BIG, {}, False, FUSED),
    "fp16_big": ("fp16", BIG, {}, False, FUSED),
    "bf16_small": ("bf16", SMALL, {}, False, UNFUSED),
    "fp32_big": ("fp32", BIG, {}, False, UNFUSED),
    "fp32_small": ("fp32", SMALL, {}, False, UNFUSED),
    "bf16_big_prune": ("bf16", BIG, dict(prune_last_block=True), False, PRUNED),
    "bf16_big_chunk32": ("bf16", BIG, dict(chunk_slices=32), False, {k: 2 * n for k, n in FUSED.items()}),
    "bf16_big_save_attn": ("bf16", BIG, {}, True, _plus(FUSED, cls_probs=DEPTH)),
    "bf16_small_save_attn": ("bf16", SMALL, {}, True, _plus(UNFUSED, cls_probs=DEPTH)),
    "fp32_small_save_attn": ("fp32", SMALL, {}, True, _plus(UNFUSED, cls_probs=DEPTH)),
    # the pruned last block reads its CLS probabilities out of its own attention launch
    "bf16_big_prune_save_attn": ("bf16", BIG, dict(prune_last_block=True), True, _plus(PRUNED, cls_probs=DEPTH - 1)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_launch_counts_and_logits(name):
    mode, shape, kw, save_attn, want = CASES[name]
    logits, counts = _profiled_forward(_model(mode, **kw), shape, save_attn)
    err = float((logits - _oracle(shape)["logits"]).abs().max())
    print(f"{name}: launches {({k: n for k, n in counts.items() if n})}; max|dlogits| vs oracle {err:.3e} (tol {TOL[mode]:g})")
    _expect(counts, want)
    assert err < TOL[mode]


@pytest.mark.parametrize("calibrated", [False, True], ids=["dynamic", "calibrated"])
@pytest.mark.parametrize("shape", [BIG, SMALL], ids=["big", "small"])
def test_fp8_launch_counts_and_embeddings(shape, calibrated):
    """fp8_linear never takes the fused pipeline, whatever the token count: LayerNorm and the four e4m3 GEMMs of every block
    are launches of their own (the quantisation launches between them carry no kind)."""
    model = _model("fp8")
    if calibrated:
        model.calibrate_fp8(_volume(shape))
    _, counts = _profiled_forward(model, shape)
    with torch.no_grad():
        emb = model.encode_slices(_volume(shape).cuda().reshape(shape[2], *shape[3:]))[0].cpu()
    exact, ref8 = _oracle(shape)["emb"], _oracle(shape, "fp8")["emb"]
    ex, e8, eq = rel_l2(emb, exact), rel_l2(emb, ref8), rel_l2(ref8, exact)
    print(f"fp8 {'calibrated' if calibrated else 'dynamic'} {shape}: launches {({k: n for k, n in counts.items() if n})}; "
          f"emb rel-L2 HIP-exact {ex:.3e}, HIP-fp8 oracle {e8:.3e}, fp8 oracle-exact {eq:.3e}")
    _expect(counts, UNFUSED)
    assert ex < 1.5 * eq and e8 < 1.5 * eq


def test_ragged_chunking_keeps_the_pipeline_and_the_logits():
    """chunk_slices=32 on 48 slices: a 32-slice chunk and a ragged 16-slice one.  The fused pipeline is chosen from the whole
    call's 12,336 tokens, so the 4,112-token last chunk stays on it; only the row layout between the blocks is a per-chunk
    decision (the blocked-input QKV kernel needs 8,192 rows)."""
    whole, _ = _profiled_forward(_model("bf16"), BIG)
    chunked, counts = _profiled_forward(_model("bf16", chunk_slices=32), BIG)
    print(f"chunk_slices=32 vs one chunk: max|dlogits| {float((whole - chunked).abs().max()):.3e}, bit-identical {torch.equal(whole, chunked)}")
    _expect(counts, {k: 2 * n for k, n in FUSED.items()})
    assert torch.equal(whole, chunked)
