"""The encoder API on the HIP path: ``model.encoder.forward`` / ``forward_features`` / ``get_intermediate_layers`` (the reference's
DinoVisionTransformer, extern/dinov2/vision_transformer.py:254-329) against the float64 restatement of tests/encoder_ref.py, which
tests/test_encoder_api_cpu.py pins to the reference's own outputs.

Bars.  Whole tensor: the project's embedding bars (tests/test_model_gpu.py TOL: fp32 2e-4, fp16 3e-3, bf16 3e-2 rel-L2), for normalised
and un-normalised outputs alike.  A whole-tensor norm hides one misplaced or stale row (one wrong row of 12,336 moves it by ~1e-2), so
every output is also held per token row: worst per-row rel-L2 <= min(0.25, 3 x CLS_ROW[case]), where CLS_ROW is the worst per-row rel-L2
of the class-token rows ``encode_slices`` (unchanged by the encoder API: the same launches, the same bits) returns for grey slices of the
same shape in the same mode, against the same restatement -- patch rows pass through the same kernels and differ only in content.
Measured on the MI355X (every test prints the value it finds beside the recorded one): CLS_ROW below, the row bars are 3 x those
(fp32 about 6e-6, fp16 4.1e-3, bf16 3.2e-2 .. 3.7e-2); the worst tapped row of every case is in MEASURED_WORST_ROW (at most 1.5 x its
CLS_ROW).  Whole-tensor figures: fp32 <= 5.6e-6, fp16 <= 1.23e-3, bf16 <= 1.26e-2.
"""
import pytest
import torch

import encoder_ref as ER
from conftest import GOLDEN, rel_l2
from mst import hip, synth
from test_model_gpu import TOL, build

pytestmark = pytest.mark.gpu

# worst per-row rel-L2 of encode_slices' class tokens against the float64 restatement, per case (shape, mode, model): measured
CLS_ROW = {
    "s_fp32_56x70": 2.160e-06, "s_fp32_28x28": 1.801e-06, "reg_fp32_56x56": 2.202e-06, "reg_fp32_56x70": 2.337e-06,
    "s_bf16_48x224": 1.073e-02, "s_fp16_48x224": 1.363e-03, "b_fp32_28x42": 2.143e-06, "b_bf16_28x42": 1.227e-02,
    "swiglu_fp32_28x28": 3.429e-06,
}
# worst per-row rel-L2 over every output of the case (recorded, not a bar)
MEASURED_WORST_ROW = {
    "s_fp32_56x70": 3.026e-06, "s_fp32_28x28": 2.115e-06, "reg_fp32_56x56": 2.576e-06, "reg_fp32_56x70": 2.805e-06,
    "s_bf16_48x224": 1.552e-02, "s_fp16_48x224": 1.883e-03, "b_fp32_28x42": 2.909e-06, "b_bf16_28x42": 1.276e-02,
    "swiglu_fp32_28x28": 5.603e-06,
}


def row_bar(key):
    return min(0.25, 3.0 * CLS_ROW[key])


def _rows(t):
    """[n, E, gh, gw] (reshape=True) back to token rows [n, gh * gw, E]; everything else as it is."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]) if t.dim() == 4 else t


IL_CALLS = (dict(n=[0, 5, 11], reshape=True, return_class_token=True), dict(n=2, norm=False), dict(n=1),
            dict(n=[3], return_class_token=True, norm=False))


def api_outputs(enc, x, il_calls=IL_CALLS):
    """{name: tensor} of every output of the three methods.  `enc`: model.encoder (x on the device) or an ER.Restated."""
    dev = isinstance(enc, torch.nn.Module)
    out = {"forward": enc(x) if dev else enc.forward()}
    ff = enc.forward_features(x) if dev else enc.forward_features()
    assert ff["masks"] is None and set(ff) == {"x_norm_clstoken", "x_norm_regtokens", "x_norm_patchtokens", "x_prenorm", "masks"}
    out.update({"ff." + k: v for k, v in ff.items() if k != "masks"})
    if dev:
        tr = enc(x, is_training=True)
        assert all(torch.equal(tr[k], ff[k]) for k in ff if k != "masks")
    for i, kw in enumerate(il_calls):
        res = enc.get_intermediate_layers(x, **kw) if dev else enc.get_intermediate_layers(**kw)
        assert isinstance(res, tuple)
        for j, r in enumerate(res):
            if kw.get("return_class_token"):
                assert isinstance(r, tuple) and len(r) == 2
                out[f"il{i}.{j}.patch"], out[f"il{i}.{j}.cls"] = r
            else:
                out[f"il{i}.{j}.patch"] = r
    return out


def figures(got, ref):
    """{name: (whole-tensor rel-L2, worst per-row rel-L2)}; shapes, dtype and device checked on the way."""
    figs = {}
    assert set(got) == set(ref)
    for k, r in ref.items():
        g = got[k]
        assert g.dtype == torch.float32 and g.is_cuda, k
        assert tuple(g.shape) == tuple(r.shape), (k, tuple(g.shape), tuple(r.shape))
        if r.numel() == 0:
            continue
        figs[k] = (rel_l2(g.cpu(), r), ER.worst_row(_rows(g), _rows(r)))
    return figs


def cls_row_baseline(model, restated_grey, grey):
    """Worst per-row rel-L2 of encode_slices' class tokens on grey [n, 1, H, W]: what CLS_ROW records."""
    with torch.no_grad():
        emb, _, _ = model.encode_slices(grey[:, 0].contiguous().cuda())
    return ER.worst_row(emb, restated_grey.forward()), emb


def run_case(key, model, sd, x, depth, heads, mode, il_calls=IL_CALLS):
    """Every output of the three methods on x against the restatement; returns (figures, outputs, restatement)."""
    ref = ER.Restated(sd, x, depth, heads)
    grey = x[:, :1]
    base, _ = cls_row_baseline(model, ref if x.shape[1] == 1 else ER.Restated(sd, grey, depth, heads), grey)
    with torch.no_grad():
        got = api_outputs(model.encoder, x.cuda(), il_calls)
    figs = figures(got, api_outputs(ref, None, il_calls))
    worst = max(figs.values(), key=lambda f: f[1])
    print(f"{key}: CLS_ROW now {base:.3e} (recorded {CLS_ROW.get(key)}); worst whole-tensor rel-L2 {max(f[0] for f in figs.values()):.3e} "
          f"(bar {TOL[mode][1]:g}); worst row {worst[1]:.3e} (bar {row_bar(key) if key in CLS_ROW else None})")
    for k, (rel, row) in figs.items():
        print(f"    {k}: rel-L2 {rel:.3e}, worst row {row:.3e}")
    return figs, got, ref


def hold(key, figs, mode):
    for k, (rel, row) in figs.items():
        assert rel < TOL[mode][1], (key, k, rel)
        assert row <= row_bar(key), (key, k, row, row_bar(key))


# ---- 1. fp32, 's', the unfused path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 56, 70), (1, 3, 28, 28)])
def test_fp32_every_output_matches_the_fp64_restatement(shape):
    model = build({}, 0, "fp32")
    x = ER.rgb_image(shape, 41)
    assert not torch.equal(x[:, 0], x[:, 1]) and not torch.equal(x[:, 1], x[:, 2])
    key = f"s_fp32_{shape[2]}x{shape[3]}"
    figs, got, _ = run_case(key, model, synth.synth_state_dict("s", 0), x, 12, 6, "fp32")
    hold(key, figs, "fp32")
    n, N = shape[0], 1 + (shape[2] // 14) * (shape[3] // 14)
    assert tuple(got["ff.x_prenorm"].shape) == (n, N, 384) and tuple(got["ff.x_norm_regtokens"].shape) == (n, 0, 384)
    assert tuple(got["il0.0.patch"].shape) == (n, 384, shape[2] // 14, shape[3] // 14) and got["il0.0.patch"].is_contiguous()
    # [n, 1, H, W]: the grey fast path -- the numbers of x.repeat(1, 3, 1, 1), the bits of encode_slices
    grey = x[:, :1].cuda()
    with torch.no_grad():
        emb, _, _ = model.encode_slices(grey[:, 0].contiguous())
        assert torch.equal(model.encoder(grey), emb)
        ff_g, ff_r = model.encoder.forward_features(grey), model.encoder.forward_features(grey.repeat(1, 3, 1, 1))
    assert torch.equal(ff_g["x_norm_clstoken"], emb)
    for k in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"):
        assert rel_l2(ff_r[k].cpu(), ff_g[k].cpu()) < TOL["fp32"][1]
        assert ER.worst_row(ff_r[k], ff_g[k]) <= row_bar(key)


def test_fp32_matches_the_reference_fixture_directly():
    """The same call as the fixture's, against the reference's own outputs (not through the restatement)."""
    import numpy as np
    with np.load(GOLDEN / "encoder_api.npz") as z:
        g = {k: z[k] for k in z.files}
    model = build({}, int(g["seed"]), "fp32")
    x = ER.rgb_image(tuple(int(v) for v in g["shape"]), int(g["image_seed"])).cuda()
    with torch.no_grad():
        ff = model.encoder.forward_features(x)
        il = model.encoder.get_intermediate_layers(x, n=[0, 5, 11], reshape=True, return_class_token=True)
    for k in ("x_norm_clstoken", "x_norm_patchtokens", "x_prenorm"):
        assert rel_l2(ff[k].cpu(), g["ff." + k]) < TOL["fp32"][1]
    for i, (patch, cls) in enumerate(il):
        assert rel_l2(patch.cpu(), g[f"il_reshape.{i}.patch"]) < TOL["fp32"][1] and rel_l2(cls.cpu(), g[f"il_reshape.{i}.cls"]) < TOL["fp32"][1]


# ---- 2. registers ----------------------------------------------------------------------------------------------------------------
def _register_model(sd):
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_registers=True)
    model.encoder = _ViT(384, 12, 6, img_size=56, num_register_tokens=4, layerscale=1.0, chunked=False)
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval()


@pytest.mark.parametrize("shape", [(2, 3, 56, 56), (2, 3, 56, 70)])
def test_register_tokens_at_the_stored_grid_and_resampled(shape):
    """56 x 56 is the stored 4 x 4 grid; 56 x 70 resamples it with the hub's anti-aliased, size-based interpolation."""
    sd = synth.synth_state_dict("s", 23, img_size=56, layerscale=True, chunked=False, num_register_tokens=4)
    model = _register_model(sd)
    x = ER.rgb_image(shape, 43)
    key = f"reg_fp32_{shape[2]}x{shape[3]}"
    figs, got, ref = run_case(key, model, sd, x, 12, 6, "fp32")
    hold(key, figs, "fp32")
    Np = (shape[2] // 14) * (shape[3] // 14)
    assert tuple(got["ff.x_norm_regtokens"].shape) == (2, 4, 384) and "ff.x_norm_regtokens" in figs
    assert tuple(got["ff.x_norm_patchtokens"].shape) == (2, Np, 384) and tuple(got["ff.x_prenorm"].shape) == (2, 5 + Np, 384)
    assert tuple(got["il1.0.patch"].shape) == (2, Np, 384)                        # patch tokens exclude the registers


# ---- 3.-6. the fused, blocked plan: 48 x 257 = 12,336 tokens, the smallest call above the 12,288-token crossover --------------------
FUSED_SHAPE = (48, 1, 224, 224)
FUSED_IL = (dict(n=[0, 5, 11], return_class_token=True),)


@pytest.fixture(scope="module")
def fused_ref():
    """One float64 restatement for every test of the fused plan (48 images x 12 blocks: seconds on the CPU); never modified."""
    n, _, H, W = FUSED_SHAPE
    x = synth.synth_volume((1, 1, n, H, W), 145)[0, 0][:, None].contiguous()
    sd = synth.synth_state_dict("s", 0)
    return x, sd, ER.Restated(sd, x, 12, 6)


def _counted(model, call):
    model.profiler = hip.Profiler()
    try:
        with torch.no_grad():
            out = call()
        counts = {k: n for k, (_, n) in model.profiler.collect().items()}
    finally:
        model.profiler = None
    return out, counts


def _fused_outputs(model, x, chunks=1):
    """get_intermediate_layers then forward_features, each under the profiler: the tap must not take the call off its plan (12 launches
    of each of the plan's three kinds per chunk of images)."""
    enc = model.encoder
    il, c1 = _counted(model, lambda: enc.get_intermediate_layers(x, **FUSED_IL[0]))
    ff, c2 = _counted(model, lambda: enc.forward_features(x))
    for c in (c1, c2):
        assert (c["block_fused"], c["gemm_qkv"], c["attention"]) == (12 * chunks, 12 * chunks, 12 * chunks), c
        assert c["gemm_fc1"] == c["gemm_fc2"] == c["gemm_proj"] == c["mlp_fused"] == 0, c
    out = {"ff." + k: v for k, v in ff.items() if k != "masks"}
    for j, (patch, cls) in enumerate(il):
        out[f"il0.{j}.patch"], out[f"il0.{j}.cls"] = patch, cls
    return out


def _fused_ref_outputs(ref):
    out = api_outputs(ref, None, FUSED_IL)
    del out["forward"]
    return out


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_fused_blocked_plan_is_kept_and_class_tokens_keep_their_bits(mode, fused_ref):
    x, sd, ref = fused_ref
    key = f"s_{mode}_48x224"
    model = build({}, 0, mode)
    xd = x.cuda()
    base, emb = cls_row_baseline(model, ref, x)
    got = _fused_outputs(model, xd)
    figs = figures(got, _fused_ref_outputs(ref))
    print(f"{key}: CLS_ROW now {base:.3e} (recorded {CLS_ROW.get(key)}); row bar {row_bar(key) if key in CLS_ROW else None}")
    for k, (rel, row) in figs.items():
        print(f"    {k}: rel-L2 {rel:.3e}, worst row {row:.3e}")
    hold(key, figs, mode)
    # the class tokens of the API are those of encode_slices, bit for bit
    assert torch.equal(got["ff.x_norm_clstoken"], emb)
    assert torch.equal(got["il0.2.cls"], emb)
    with torch.no_grad():
        assert torch.equal(model.encoder(xd), emb)
    # true RGB input on the same plan; three identical channels give the grey numbers within the bars
    rgb = _fused_outputs(model, xd.repeat(1, 3, 1, 1))
    figs_rgb = figures(rgb, _fused_ref_outputs(ref))
    hold(key, figs_rgb, mode)
    for k, v in rgb.items():
        if v.numel() == 0:
            continue
        rel, row = rel_l2(v.cpu(), got[k].cpu()), ER.worst_row(_rows(v), _rows(got[k]))
        print(f"    rgb vs grey {k}: rel-L2 {rel:.3e}, worst row {row:.3e}")
        assert rel < TOL[mode][1] and row <= row_bar(key), (k, rel, row)


def test_chunked_calls_give_the_bits_of_the_unchunked_call(fused_ref):
    """chunk_slices=32: chunks of 32 and 16 images.  Grey and true RGB (three different channels: the chunk offset counts channels)."""
    x, _, _ = fused_ref
    whole, chunked = build({}, 0, "bf16"), build({}, 0, "bf16", chunk_slices=32)
    rgb = torch.cat([x, x.flip(0), x.flip(3)], dim=1).contiguous()
    for inp in (x.cuda(), rgb.cuda()):
        a, b = _fused_outputs(whole, inp), _fused_outputs(chunked, inp, chunks=2)
        for k in a:
            assert torch.equal(a[k], b[k]), k
        with torch.no_grad():
            assert torch.equal(whole.encoder(inp), chunked.encoder(inp))


@pytest.mark.parametrize("plan", ["fused_bf16", "unfused_fp32"])
def test_nothing_is_written_beyond_the_tap_rows(plan, fused_ref):
    """hip.vit_encode_features with `out` carved out of a larger zeroed tensor."""
    if plan == "fused_bf16":
        model, x = build({}, 0, "bf16"), fused_ref[0].cuda()
    else:
        model, x = build({}, 0, "fp32"), ER.rgb_image((2, 3, 56, 70), 41).cuda()
    blocks = [0, 5, 11]
    with torch.no_grad():
        _, want = model.encode_features(x, blocks, True, False)                    # also leaves the struct prepared for this shape
    vit = model._prepare()["vit"]
    n, ch, H, W = x.shape
    N, E, guard = want.shape[2], 384, 8192
    big = torch.zeros(2 * guard + want.numel(), dtype=torch.float32, device="cuda")
    out = big[guard:guard + want.numel()].view(len(blocks), n, N, E)
    ws = hip.workspace(hip.vit_features_workspace_bytes(vit, ch, H, W, n), x.device)
    wrgb = hip.pack_patch_rgb(model.encoder.patch_embed.proj.weight, torch.float32) if ch == 3 else None
    hip.vit_encode_features(vit, x[:, 0].contiguous() if ch == 1 else x, n, ws, patch_w_rgb=wrgb, blocks=blocks, norm=True, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert float(big[:guard].abs().max()) == 0.0 and float(big[guard + want.numel():].abs().max()) == 0.0
    with pytest.raises(RuntimeError, match="workspace"):
        hip.vit_encode_features(vit, x[:, 0].contiguous() if ch == 1 else x, n, ws[:1024], patch_w_rgb=wrgb, blocks=blocks, norm=True, out=out)
    with pytest.raises(RuntimeError, match="ascending"):
        hip.vit_encode_features(vit, x[:, 0].contiguous() if ch == 1 else x, n, ws, patch_w_rgb=wrgb, blocks=[5, 0, 11], norm=True, out=out)


@pytest.mark.parametrize("plan", ["fused_bf16", "unfused_fp32"])
def test_prune_last_block_does_not_change_the_features(plan, fused_ref):
    """A tapped call never prunes: the pruned last block has no patch rows."""
    mode = "bf16" if plan == "fused_bf16" else "fp32"
    x = fused_ref[0].cuda() if plan == "fused_bf16" else ER.rgb_image((2, 3, 56, 70), 41).cuda()
    plain, pruned = build({}, 0, mode), build({}, 0, mode, prune_last_block=True)
    with torch.no_grad():
        a, b = plain.encoder.forward_features(x), pruned.encoder.forward_features(x)
    for k in ("x_norm_clstoken", "x_norm_regtokens", "x_norm_patchtokens", "x_prenorm"):
        assert torch.equal(a[k], b[k]), k


# ---- 7. model variants -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_model_size_b(mode):
    model = build(dict(model_size="b"), 6, mode)
    key = f"b_{mode}_28x42"
    figs, got, _ = run_case(key, model, synth.synth_state_dict("b", 6), ER.rgb_image((1, 3, 28, 42), 47), 12, 12, mode)
    hold(key, figs, mode)
    assert tuple(got["ff.x_prenorm"].shape) == (1, 7, 768)


def test_swiglu_blocks(mode="fp32"):
    """SwiGLU blocks in fp32, the mode in which this 12-block SwiGLU model (no LayerScale) is inside the project's bars at all.  In the
    16-bit modes the UNCHANGED class-token path misses the whole-tensor bars on this model by itself: encode_slices on twelve grey
    1 x 28 x 28 inputs against the same restatement measured 1.77e-2 .. 3.16e-2 in bf16 (bar 3e-2) and 2.31e-3 .. 3.58e-3 in fp16 (bar
    3e-3); the encoder API on RGB inputs sits in the same band (forward: 1.91e-2 .. 3.02e-2 bf16, 2.43e-3 .. 4.20e-3 fp16; worst tapped
    row 3.02e-2 against a row bar of 5.8e-2).  The error grows block by block (6e-3, 2.1e-2, 3.0e-2 behind blocks 0, 5, 11): it is the
    16-bit block pipeline's accumulation, not the patch embedding's or the taps'.  A 16-bit case here would test that, not this API; the
    16-bit modes are held on the GELU models above ('s' fused plan, 'b')."""
    from mst.models import DinoV2ClassifierSlice
    sd = synth.synth_state_dict("s", 32, ffn_layer="swiglufused")
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode, ffn_layer="swiglufused")
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    key = f"swiglu_{mode}_28x28"
    figs, _, _ = run_case(key, model, sd, ER.rgb_image((1, 3, 28, 28), 49), 12, 6, mode)
    hold(key, figs, mode)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    x = torch.zeros(1, 3, 28, 28, device="cuda")
    fp8 = build({}, 0, "fp8")
    with torch.no_grad():
        for call in (lambda: fp8.encoder(x), lambda: fp8.encoder.forward_features(x), lambda: fp8.encoder.get_intermediate_layers(x)):
            with pytest.raises(NotImplementedError, match="fp8"):
                call()
    model = build({}, 0, "fp32")
    assert torch.is_grad_enabled() and any(p.requires_grad for p in model.encoder.parameters())
    for call in (lambda: model.encoder(x), lambda: model.encoder.forward_features(x), lambda: model.encoder.get_intermediate_layers(x, n=2)):
        with pytest.raises(NotImplementedError, match="no_grad"):                    # a trainable encoder with grad enabled
            call()
    for p in model.parameters():
        p.requires_grad_(False)
    assert model.encoder(x).shape == (1, 384)                                       # frozen: nothing asks for a gradient
    with pytest.raises(NotImplementedError, match="no_grad"):                        # ... until the input does
        model.encoder.forward_features(x.clone().requires_grad_(True))
    with torch.no_grad():
        out = model.encoder.forward_features(x.clone().requires_grad_(True))         # under no_grad nothing is refused
        assert not out["x_prenorm"].requires_grad
        with pytest.raises(NotImplementedError, match="mask"):
            model.encoder.forward_features(x, masks=torch.zeros(1, 4, dtype=torch.bool))
        with pytest.raises(NotImplementedError, match="list"):
            model.encoder.forward_features([x])
        import json
        msg = json.loads((GOLDEN / "errors.json").read_text())["512x512"]["message"]
        with pytest.raises(AssertionError) as e:
            model.encoder.forward_features(torch.zeros(1, 3, 512, 512, device="cuda"))
        assert str(e.value) == msg
        with pytest.raises(AssertionError, match=r"only 1 / 2 blocks found"):
            model.encoder.get_intermediate_layers(x, n=[3, 12])
