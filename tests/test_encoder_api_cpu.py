"""The encoder API (model.encoder.forward / forward_features / get_intermediate_layers) without a GPU: the restatement the GPU tests
compare against is pinned to the reference's own DinoVisionTransformer; the C ABI additions are declared, bound and exported; the
refusals that must come before any device check come in their order; the encoder's link to its model survives replacement and
deepcopy without touching the state dict."""
import copy
import ctypes
import re

import pytest
import torch

import encoder_ref as ER
from conftest import ROOT, load_golden, rel_l2
from mst import hip, synth
from mst.models import DinoV2ClassifierSlice
from mst.models.dino import _ViT

FIXTURE_BAR = 1e-5      # the project's oracle-vs-fixture bar (the oracle's noise floor is 2.4e-7)


@pytest.fixture(scope="module")
def restated():
    g = load_golden("encoder_api")
    shape = tuple(int(v) for v in g["shape"])
    assert shape == (2, 3, 56, 70)
    x = ER.rgb_image(shape, int(g["image_seed"]))
    assert not torch.equal(x[:, 0], x[:, 1]) and not torch.equal(x[:, 1], x[:, 2])        # three different channels
    return g, ER.Restated(synth.synth_state_dict("s", int(g["seed"])), x, 12, 6, dtype=torch.float32)


def test_restatement_forward_features_matches_the_reference_fixture(restated):
    g, r = restated
    ff = r.forward_features()
    assert ff["masks"] is None and tuple(ff["x_norm_regtokens"].shape) == (2, 0, 384)
    for k in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"):
        assert tuple(ff[k].shape) == g["ff." + k].shape
        err = rel_l2(ff[k], g["ff." + k])
        print(k, err)
        assert err < FIXTURE_BAR, (k, err)
    assert g["ff.x_norm_regtokens"].shape == (2, 0, 384)
    assert rel_l2(r.forward(), g["forward"]) < FIXTURE_BAR


def test_restatement_intermediate_layers_match_the_reference_fixture(restated):
    g, r = restated
    assert g["il_blocks"].tolist() == [0, 5, 11]
    got = r.get_intermediate_layers(n=[0, 5, 11], reshape=True, return_class_token=True)
    assert len(got) == 3
    for i, (patch, cls) in enumerate(got):
        assert tuple(patch.shape) == (2, 384, 4, 5) and patch.is_contiguous()
        assert rel_l2(patch, g[f"il_reshape.{i}.patch"]) < FIXTURE_BAR
        assert rel_l2(cls, g[f"il_reshape.{i}.cls"]) < FIXTURE_BAR
    last2 = r.get_intermediate_layers(n=2, norm=False)
    assert len(last2) == 2
    for i, patch in enumerate(last2):
        assert tuple(patch.shape) == (2, 20, 384)
        assert rel_l2(patch, g[f"il_last2_prenorm.{i}"]) < FIXTURE_BAR
    with pytest.raises(AssertionError, match=r"only 1 / 2 blocks found"):
        r.get_intermediate_layers(n=[3, 12])


def test_abi_additions_are_declared_bound_and_exported():
    header = (ROOT / "include" / "mst_hip.h").read_text()
    assert re.search(r"^size_t\s+mst_vit_features_workspace_bytes\s*\(const mst_vit_weights\* w, int in_channels, int H, int W, int chunk_images\);",
                     header, flags=re.M)
    m = re.search(r"^int\s+mst_vit_encode_features\s*\(([^;]*)\);", header, flags=re.M)
    assert m, "mst_vit_encode_features is not declared"
    args = [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]
    assert args == ["const mst_vit_weights* w", "const void* img", "int in_dtype", "int in_channels", "int n_images", "int H", "int W",
                    "const void* patch_w_rgb", "float* cls_out", "const mst_vit_taps* taps", "int chunk_images", "void* ws", "size_t ws_bytes",
                    "mst_stream_t stream"]
    t = re.search(r"typedef struct mst_vit_taps \{(.*?)\} mst_vit_taps;", header, flags=re.S)
    assert t and [f.split()[-1].strip("*;") for f in re.findall(r"^\s*(?:const )?(?:int|float)\*? \w+;", t.group(1), flags=re.M)] == \
        ["n_taps", "blocks", "norm", "out"]
    i, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    W = ctypes.POINTER(hip.VitWeights)
    assert hip.SIGNATURES["mst_vit_features_workspace_bytes"] == (sz, [W, i, i, i, i])
    assert hip.SIGNATURES["mst_vit_encode_features"] == (i, [W, vp, i, i, i, i, i, vp, vp, ctypes.POINTER(hip.VitTaps), i, vp, sz, vp])
    assert [(n, t) for n, t in hip.VitTaps._fields_] == [("n_taps", i), ("blocks", ctypes.POINTER(i)), ("norm", i), ("out", vp)]
    lib = hip.load()
    assert hasattr(lib, "mst_vit_encode_features") and hasattr(lib, "mst_vit_features_workspace_bytes")
    assert lib.mst_version() == 300 == hip.ABI_VERSION
    # host-side argument checks run before anything touches a device
    w = hip.VitWeights()
    assert lib.mst_vit_features_workspace_bytes(ctypes.byref(w), 2, 28, 28, 1) == 0
    assert lib.mst_vit_encode_features(ctypes.byref(w), None, hip.F32, 2, 1, 28, 28, None, None, None, 1, None, 0, None) != 0
    assert "in_channels=2" in hip.last_error()
    assert lib.mst_vit_encode_features(ctypes.byref(w), None, hip.F32, 3, 1, 28, 28, None, None, None, 1, None, 0, None) != 0
    assert "patch_w_rgb" in hip.last_error()


def test_pack_patch_rgb_image():
    w = torch.randn(8, 3, 14, 14)
    img = hip.pack_patch_rgb(w, torch.float32)
    assert tuple(img.shape) == (8, 672)
    v = img.view(8, 3, 14, 16)
    assert torch.equal(v[..., :14], w) and float(v[..., 14:].abs().max()) == 0.0
    assert hip.pack_patch_rgb(w, torch.bfloat16).dtype == torch.bfloat16


def test_refusals_on_a_cpu_model_come_in_order():
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False).eval()
    enc = model.encoder
    x = torch.zeros(1, 3, 28, 28)
    assert enc.n_blocks == 12 and enc.chunked_blocks is True
    # masks, then list input: raised before any device check, although this model has no device to run on and asks for gradients
    with pytest.raises(NotImplementedError, match="mask"):
        enc.forward_features(x, masks=torch.zeros(1, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="mask"):
        enc(x, masks=torch.zeros(1, 4, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="list"):
        enc.forward_features([x, x], None)
    with pytest.raises(NotImplementedError, match="list"):
        enc.forward_features_list([x], [None])
    # then the device: grad is enabled and the parameters are trainable, yet the CPU refusal comes first
    assert torch.is_grad_enabled() and any(p.requires_grad for p in enc.parameters())
    for call in (lambda: enc(x), lambda: enc(x, is_training=True), lambda: enc.forward_features(x),
                 lambda: enc.get_intermediate_layers(x, n=4)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(AssertionError, match=r"only 1 / 2 blocks found"):
        enc.get_intermediate_layers(x, n=[3, 12])


def test_the_encoder_belongs_to_its_model():
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False)
    keys = list(model.state_dict())
    modules = [n for n, _ in model.named_modules()]
    assert model.encoder._owner() is model
    # replacing the encoder (tests/test_input_grad_gpu.py, tests/test_swiglu_*.py do) re-links the new one
    new = _ViT(384, 12, 6, img_size=56, num_register_tokens=4, layerscale=1.0, chunked=False)
    assert new._owner() is None
    old = model.encoder
    model.encoder = new
    assert model.encoder is new and new._owner() is model
    assert not any("_owner" in k for k in model.state_dict()) and not any("_owner" in n for n, _ in model.named_modules())
    assert set(model.state_dict()) == set(synth.synth_state_dict("s", 0, img_size=56, layerscale=True, chunked=False, num_register_tokens=4))
    model.encoder = old
    assert list(model.state_dict()) == keys and [n for n, _ in model.named_modules()] == modules
    # a copy's encoder serves the copy; the copy has the same keys and its own parameters
    twin = copy.deepcopy(model)
    assert twin is not model and twin.encoder is not model.encoder
    assert twin.encoder._owner() is twin and model.encoder._owner() is model
    assert list(twin.state_dict()) == keys
    assert twin.encoder.cls_token.data_ptr() != model.encoder.cls_token.data_ptr()
    # a copy of the encoder alone belongs to nobody until it is assigned
    assert copy.deepcopy(model.encoder)._owner() is None
