"""model_size='g' and the SwiGLU FFN (ffn_layer='swiglufused'), the parts that need no GPU: the CPU reference of tests/swiglu_ref.py against
the fixtures the REFERENCE produced (tools/gen_golden.py: swiglu_ops, swiglu_s2, swiglu_g1, hub_vitg14_keys), the constructor (key layout,
the ffn_layer table, its refusals, meta-device construction), the weight image of the fused epilogue, the synthetic weights, the C ABI, and
the arithmetic of the 16-bit training modes emulated in float64."""
import ctypes
import json
import re

import pytest
import torch

import swiglu_ref as R
from conftest import GOLDEN, ROOT, load_golden, rel_l2
from mst import hip, synth
from mst.models import DinoV2ClassifierSlice
from mst.models.dino import _ViT, resolve_ffn_layer

# rel-L2 of the composition against the reference's fixtures: about 10x the reference's own float32 noise (its float32 run against its
# float64 run: 1.7e-6; this composition against the live reference: 1.9e-6 at E = 384 depth 2, 6.5e-7 at E = 1536 depth 1)
FIXTURE_BAR = 2e-5


def _ffn_weights(E, seed, stream):
    H = R.hidden_of(E)
    n = lambda shape, k: torch.from_numpy(synth.hash_normal(shape, seed, stream + k))
    return (n((2 * H, E), 1) * (1.2 / E ** 0.5), n((2 * H,), 2) * 0.3, n((E, H), 3) * (0.9 / H ** 0.5), n((E,), 4) * 0.05), H


def _meta_model(**kw):
    with torch.device("meta"):
        return DinoV2ClassifierSlice(in_ch=1, out_ch=2, **kw)


# ---- the helper against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,E", [("384", 384), ("128", 128)])
def test_helper_ffn_matches_reference_fixture(tag, E):
    g = load_golden("swiglu_ops")
    (w12, b12, w3, b3), H = _ffn_weights(E, int(g["seed"]), int(g[f"stream_{tag}"]))
    assert H == int(g[f"hidden_{tag}"]) == {384: 1024, 128: 344}[E]
    x = torch.from_numpy(synth.hash_normal((int(g[f"rows_{tag}"]), E), int(g["seed"]), int(g[f"stream_{tag}"]) + 5))
    assert rel_l2(R.swiglu_ffn(x, w12, b12, w3, b3), g[f"out_{tag}"]) < FIXTURE_BAR


def test_helper_encoder_matches_reference_fixtures():
    g = load_golden("swiglu_s2")
    seed = int(g["seed"])
    sd = synth.synth_state_dict("s", seed, img_size=518, layerscale=True, chunked=False, ffn_layer="swiglufused", depth=2)
    with torch.no_grad():
        for tag in ("3x28x42", "2x224x224"):
            x = synth.synth_volume((1, 1) + tuple(int(v) for v in g[f"shape_{tag}"]), seed + 100)[0, 0]
            assert rel_l2(R.encode(sd, x, 2, 6)[0], g[f"emb_{tag}"]) < FIXTURE_BAR, tag
        src = synth.synth_volume(tuple(int(v) for v in g["model_shape"]), seed + 101)
        out = R.forward(sd, src, 2, 6, keep="cls")
    from oracle import mst_oracle as O
    assert rel_l2(out["logits"], g["logits"]) < FIXTURE_BAR
    assert rel_l2(torch.stack([m[:, :, 0] for m in out["vit_maps"]]), g["vit_cls_rows"]) < FIXTURE_BAR
    assert rel_l2(out["slice_map"], g["slice_map"]) < FIXTURE_BAR
    assert rel_l2(O.plane_attention(out["vit_maps"][-1]), g["plane_attention"]) < FIXTURE_BAR
    assert rel_l2(O.slice_attention(out["slice_map"]), g["slice_attention"]) < FIXTURE_BAR
    assert rel_l2(O.attention_maps(out["vit_maps"][-1], out["slice_map"]), g["attention_maps"]) < FIXTURE_BAR


def test_helper_g_width_encoder_matches_reference_fixture():
    g = load_golden("swiglu_g1")
    seed = int(g["seed"])
    sd = synth.synth_state_dict("g", seed, img_size=518, layerscale=True, chunked=False, ffn_layer="swiglufused", depth=1)
    x = synth.synth_volume((1, 1) + tuple(int(v) for v in g["shape"]), seed + 100)[0, 0]
    with torch.no_grad():
        assert rel_l2(R.encode(sd, x, 1, 24)[0], g["emb"]) < FIXTURE_BAR


# ---- constructor -----------------------------------------------------------------------------------------------------------------------
def test_meta_built_g_model_has_the_hub_key_layout():
    """The hub layout of dinov2_vitg14 (SwiGLU, LayerScale, 518 grid, unchunked) as the pretrained=True branch builds it, without the
    download: the encoder class the branch constructs, on the meta device, against the reference's own key list."""
    want = {k: tuple(v) for k, v in json.loads((GOLDEN / "hub_vitg14_keys.json").read_text()).items()}
    with torch.device("meta"):
        enc = _ViT(1536, 40, 24, img_size=518, num_register_tokens=0, layerscale=1.0, chunked=False, ffn_layer="swiglufused")
    got = {k: tuple(v.shape) for k, v in enc.state_dict().items()}
    assert got == want
    assert got["blocks.39.mlp.w12.weight"] == (8192, 1536) and got["blocks.39.mlp.w3.weight"] == (1536, 4096)


def test_meta_built_g_model_has_the_chunked_mlp_layout_of_the_synthetic_weights():
    m = _meta_model(pretrained=False, model_size="g")
    assert all(p.is_meta for p in m.parameters()) and sum(p.numel() for p in m.parameters()) > 1.1e9
    assert m.ffn_layer == "mlp" and m.encoder.embed_dim == 1536 and m.encoder.num_heads == 24 and m.encoder.depth == 40
    # one block of 40 is synthesised (each block's tensors are a function of their own key): every block has block 0's shapes
    sd = synth.synth_state_dict("g", 0, depth=1)
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: s for k, s in got.items() if not re.match(r"encoder\.blocks\.0\.([1-9]\d*)\.", k)}
    for i in (1, 39):
        assert {k.replace(".0.0.", f".0.{i}."): tuple(v.shape) for k, v in sd.items() if ".blocks.0.0." in k}.items() <= got.items()
    assert got["encoder.blocks.0.39.mlp.fc1.weight"] == (6144, 1536)


def test_reduced_depth_swiglu_model_builds_on_meta_and_loads_strictly():
    m = _meta_model(pretrained=False, model_size="g", ffn_layer="swiglufused")
    with torch.device("meta"):
        m.encoder = _ViT(1536, 1, 24, img_size=224, chunked=True, ffn_layer="swiglufused")
    m = m.to_empty(device="cpu")
    sd = synth.synth_state_dict("g", 5, depth=1, ffn_layer="swiglufused")
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.encoder.blocks[0][0].mlp.w12.weight, sd["encoder.blocks.0.0.mlp.w12.weight"])
    # the other block layout loads too (hub <-> chunked remap)
    hub = {k.replace("encoder.blocks.0.", "encoder.blocks."): v for k, v in sd.items()}
    m.load_state_dict(hub, strict=True)


@pytest.mark.parametrize("ffn,pretrained,size,want", [
    (None, False, "s", "mlp"), (None, False, "g", "mlp"), (None, True, "s", "mlp"), (None, True, "b", "mlp"), (None, True, "g", "swiglufused"),
    ("mlp", True, "g", "mlp"), ("swiglufused", False, "s", "swiglufused"), ("swiglu", False, "g", "swiglufused"), ("SwiGLU", False, "b", "swiglufused")])
def test_ffn_layer_resolution(ffn, pretrained, size, want):
    assert resolve_ffn_layer(ffn, pretrained, size) == want
    if not pretrained:
        m = _meta_model(pretrained=False, model_size=size, ffn_layer=ffn)
        assert m.ffn_layer == want and hasattr(m.encoder.block_list()[0].mlp, "w12") == (want == "swiglufused")


def test_refusals_are_clear():
    with pytest.raises(ValueError, match="ffn_layer must be None or one of"):
        _meta_model(pretrained=False, ffn_layer="geglu")
    with pytest.raises(NotImplementedError, match="fp8.*no SwiGLU form"):
        _meta_model(pretrained=False, ffn_layer="swiglufused", compute_dtype="fp8")
    with pytest.raises(NotImplementedError, match="fp8.*embed_dim 1024"):
        _meta_model(pretrained=False, model_size="g", compute_dtype="fp8")
    with pytest.raises(ValueError, match="ffn_layer"):
        synth.synth_state_dict("s", 0, ffn_layer="geglu")
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.swiglu_fwd(torch.zeros(2, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        hip.swiglu_bwd(torch.zeros(2, 16), torch.zeros(2, 8))


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
def test_synth_defaults_are_unchanged_and_swiglu_only_changes_the_ffn():
    want = json.loads((GOLDEN / "weights.json").read_text())
    assert synth.state_dict_digest(synth.synth_state_dict("s", 0)) == want["s_seed0"]
    base = synth.synth_state_dict("s", 3, depth=2)
    full = synth.synth_state_dict("s", 3)
    assert all(torch.equal(v, full[k]) for k, v in base.items()) and len(base) < len(full)
    sw = synth.synth_state_dict("s", 3, depth=2, ffn_layer="swiglu")
    assert set(sw) ^ set(base) == {f"encoder.blocks.0.{i}.mlp.{n}.{p}" for i in (0, 1) for n in ("fc1", "fc2", "w12", "w3") for p in ("weight", "bias")}
    assert all(torch.equal(v, base[k]) for k, v in sw.items() if k in base)
    assert sw["encoder.blocks.0.1.mlp.w12.weight"].shape == (2048, 384) and sw["encoder.blocks.0.1.mlp.w3.weight"].shape == (384, 1024)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("E", [128, 384])
def test_pack_swiglu_image(E, dtype):
    """Un-pairing the image gives back w12 and w3 (rounded to the operand type), the padding is zero, and the pairing is the one
    include/mst_hip.h states: image rows 2G g + [0, G) = w12 rows G g + [0, G), image rows 2G g + G + [0, G) = w12 rows Hp + G g + [0, G)."""
    (w12, b12, w3, _), H = _ffn_weights(E, 9, 0)
    w12p, b12p, w3p = hip.pack_swiglu(w12, b12, w3, dtype)
    G, Hp = hip.swiglu_group(dtype), (H + 63) // 64 * 64
    assert G == (32 if dtype == torch.float32 else 16)
    assert w12p.shape == (2 * Hp, E) and w12p.dtype == dtype and b12p.shape == (2 * Hp,) and b12p.dtype == torch.float32
    assert w3p.shape == (E, Hp) and w3p.dtype == dtype
    assert torch.equal(R.unpair(w12p, H, G), w12.to(dtype)) and torch.equal(R.unpair(b12p, H, G), b12)
    assert torch.equal(w3p[:, :H], w3.to(dtype)) and not bool(w3p[:, H:].any())
    padded = torch.zeros(2, Hp, E)
    padded[:, :H] = w12.view(2, H, E)
    for g in range(Hp // G):
        assert torch.equal(w12p[2 * G * g:2 * G * g + G].float(), padded[0, G * g:G * g + G].to(dtype).float())
        assert torch.equal(w12p[2 * G * g + G:2 * G * (g + 1)].float(), padded[1, G * g:G * g + G].to(dtype).float())
    if Hp > H:                                                           # E = 128: H = 344 pads to 384; the padded gates and values are zero rows
        full = R.unpair(w12p, Hp, G).view(2, Hp, E)
        assert not bool(full[:, H:].any()) and not bool(R.unpair(b12p, Hp, G).view(2, Hp)[:, H:].any())
    # the padded image computes the same FFN
    x = torch.from_numpy(synth.hash_normal((5, E), 9, 50))
    pre = x @ R.unpair(w12p, Hp, G).float().t() + R.unpair(b12p, Hp, G)
    got = (R.silu(pre[:, :Hp]) * pre[:, Hp:]) @ w3p.float().t()
    want = R.swiglu_ffn(x, w12.to(dtype).float(), b12, w3.to(dtype).float(), None)
    assert rel_l2(got, want) < 1e-6


def test_pack_swiglu_refuses_mismatched_shapes():
    with pytest.raises(ValueError, match="pack_swiglu"):
        hip.pack_swiglu(torch.zeros(16, 8), torch.zeros(16), torch.zeros(8, 7), torch.float32)


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_version_stays_and_the_new_symbols_are_exported():
    lib = hip.load()
    assert lib.mst_version() == 300 == hip.ABI_VERSION
    header = (ROOT / "include" / "mst_hip.h").read_text()
    for name in ("mst_swiglu_fwd", "mst_swiglu_bwd", "mst_swiglu_fwd16", "mst_swiglu_bwd16"):
        assert name in hip.SIGNATURES and hasattr(lib, name) and re.search(rf"\bint {name}\(", header), name
    assert "MST_EPI_BIAS_SWIGLU = 5" in header and hip.EPI_BIAS_SWIGLU == 5
    # the two fields sit at the tail of mst_vit_weights, behind prune_last_block: a zero-initialised struct is the MLP
    names = [f[0] for f in hip.VitWeights._fields_]
    assert names[-3:] == ["prune_last_block", "ffn_kind", "ffn_hidden"]
    assert re.search(r"int prune_last_block;.*?int ffn_kind;.*?int ffn_hidden;[^;]*\} mst_vit_weights;", header, re.S)
    w = hip.VitWeights()
    assert w.ffn_kind == hip.FFN_MLP == 0 and w.ffn_hidden == 0
    assert hip.VitWeights.ffn_kind.offset == hip.VitWeights.prune_last_block.offset + ctypes.sizeof(ctypes.c_int)
    assert "ffn_kind" not in [f[0] for f in hip.VitLayer._fields_]             # mst_vit_layer keeps its stride


# ---- the arithmetic of the 16-bit training modes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,bars", [("fp16", (1e-2, 8e-3)), ("bf16", (1.3e-1, 7e-2))])
def test_16bit_arithmetic_alone_stays_inside_the_training_bars(prec, bars):
    """The SwiGLU hidden value is a product of two rounded factors, so that the 16-bit step of this encoder fits the bars of
    tests/test_train_storage_gpu.py (per parameter and logits, global rel-L2) is not a given: the helper in float64 with every operand
    rounded where the kernels round it (E = 384, depth 2, LayerScale, (1, 1, 4, 224, 224)) against the unrounded float64 run.
    Measured: fp16 flash 8.1e-4 / 2.5e-3 / 2.2e-3, fp16 16-bit storage 1.1e-3 / 3.0e-3 / 2.6e-3, bf16 flash 1.9e-2 / 3.7e-2 / 3.1e-2,
    bf16 16-bit storage 2.1e-2 / 3.4e-2 / 3.0e-2 (logits / worst parameter / global): inside the bars with a factor 2.7 (fp16) and 2.2
    (bf16) to spare, so tests/test_swiglu_gpu.py keeps them."""
    dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[prec]
    sd = synth.synth_state_dict("s", 32, img_size=518, layerscale=True, chunked=False, ffn_layer="swiglufused", depth=2)
    src, tgt = synth.synth_volume((1, 1, 4, 224, 224), 3), torch.tensor([1])
    _, l0, g0 = R.grads(sd, src, 2, 6, tgt)
    keys = [k for k, v in g0.items() if v is not None and k != "<source>"]
    for storage16 in (False, True):
        _, l1, g1 = R.grads(sd, src, 2, 6, tgt, round16=dt, storage16=storage16)
        d = float((l1 - l0).abs().max())
        worst = max(rel_l2(g1[k], g0[k]) for k in keys)
        glob = (sum(float((g1[k] - g0[k]).square().sum()) for k in keys) / sum(float(g0[k].square().sum()) for k in keys)) ** 0.5
        print(f"{prec} storage16={storage16}: logits {d:.2e} worst {worst:.2e} global {glob:.2e}")
        assert d < bars[0] and worst < bars[0] and glob < bars[1], (d, worst, glob)
