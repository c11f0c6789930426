"""model_size='g' and the SwiGLU FFN on the MI355X: the fused GEMM epilogue (MST_EPI_BIAS_SWIGLU of csrc/k_gemm16.hip and k_gemm32.hip) and the row
kernels of the training step (mst_swiglu_fwd / _bwd and their 16-bit forms) against float64, inference in the three compute types against
the fixtures the REFERENCE produced (tools/gen_golden.py: swiglu_ops, swiglu_s2, swiglu_g1) and against the CPU oracle at the 'g' width, and the
training step against float64 autograd through tests/swiglu_ref.py."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

import swiglu_ref as R
import train_parity as P
from conftest import load_golden, rel_l2
from mst import hip, synth
from test_attn_train_gpu import _compare
from test_hip_ops import OUT_TOL, rnd, scaled_err
from test_model_gpu import TOL

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _swiglu64(a, w12, b12):
    pre = a.double() @ w12.double().t() + b12.double()
    H = w12.shape[0] // 2
    return pre[:, :H] * torch.sigmoid(pre[:, :H]) * pre[:, H:]


def _operands(M, H, K, tdt, seed=40):
    a = rnd((M, K), seed).to(tdt)
    w12 = (rnd((2 * H, K), seed + 1) / math.sqrt(K)).to(tdt)
    b12 = rnd((2 * H,), seed + 2) * 0.1
    return a, w12, b12


def _packed(w12, b12, tdt):
    H, K = w12.shape[0] // 2, w12.shape[1]
    w12p, b12p, _ = hip.pack_swiglu(w12.cuda(), b12.cuda(), torch.zeros(K, H, device="cuda"), tdt)
    return w12p, b12p


# ---- the epilogue -----------------------------------------------------------------------------------------------------------------------
# (130, 64, 64): one ragged row tile, a single K stage; (257, 192, 192): the LDS ring wraps; (1030, 1792, 384): 9 x 28 = 252 tiles of
# 128 x 128 (>= 224: the wide tile; the others take 128 x 64); (300, 344, 128): H pads to 384
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("M,H,K", [(130, 64, 64), (257, 192, 192), (1030, 1792, 384), (300, 344, 128)])
def test_swiglu_epilogue_16bit(dt, M, H, K):
    tdt = DT[dt]
    a, w12, b12 = _operands(M, H, K, tdt)
    ref = _swiglu64(a, w12, b12)
    w12p, b12p = _packed(w12, b12, tdt)
    Hp = w12p.shape[0] // 2
    assert Hp == (H + 63) // 64 * 64
    for odt in (tdt, torch.float32):
        got = hip.gemm(a.cuda(), w12p, b12p, epilogue=hip.EPI_BIAS_SWIGLU, out_dtype=odt)
        assert got.shape == (M, Hp) and got.dtype == odt
        err = scaled_err(got[:, :H], ref)
        print(f"swiglu epilogue {dt} -> {odt} ({M}, {H}, {K}): {err:.3e}")
        assert err < OUT_TOL[odt], (odt, err)
        assert not bool(got[:, H:].any())                                # zero gate rows and zero value rows: silu(0) * 0


@pytest.mark.parametrize("M,H,K", [(130, 64, 64), (257, 192, 192)])
def test_swiglu_epilogue_fp32(M, H, K):
    a, w12, b12 = _operands(M, H, K, torch.float32, 50)
    w12p, b12p = _packed(w12, b12, torch.float32)
    got = hip.gemm(a.cuda(), w12p, b12p, epilogue=hip.EPI_BIAS_SWIGLU)
    assert got.shape == (M, H) and got.dtype == torch.float32
    assert scaled_err(got, _swiglu64(a, w12, b12)) < 2e-5


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("M,H", [(130, 192), (1030, 1792)])
def test_swiglu_epilogue_pairs_gate_and_value_of_the_same_column(dt, M, H):
    """Every gate is the constant 1 (A[:, 1] = 1 against w12[j][1] = 1) and the value of column j is the integer j % 251 (A[:, 0] = 1
    against w12[H + j][0], exact in bf16): the output is silu(1) * (j % 251), and a wrong pairing map an error of order 1.  Both tile widths."""
    tdt, K = DT[dt], 64
    a = torch.zeros(M, K)
    a[:, :2] = 1.0
    w12 = torch.zeros(2 * H, K)
    w12[:H, 1] = 1.0
    w12[H:, 0] = (torch.arange(H) % 251).float()
    w12p, b12p = _packed(w12, torch.zeros(2 * H), tdt)
    got = hip.gemm(a.to(tdt).cuda(), w12p, b12p, epilogue=hip.EPI_BIAS_SWIGLU, out_dtype=torch.float32)
    want = (1.0 / (1.0 + math.exp(-1.0))) * (torch.arange(H) % 251).double().expand(M, H)
    assert float((got.cpu().double() - want).abs().max()) < 1e-3, float((got.cpu().double() - want).abs().max())


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_swiglu_epilogue_refuses_an_image_that_is_not_whole_pairing_groups(dt):
    tdt = DT[dt]
    a = torch.zeros(8, 64, dtype=tdt, device="cuda")
    w = torch.zeros(96, 64, dtype=tdt, device="cuda")                      # 96 image rows: not a multiple of 128
    out = torch.full((8, 48), 7.0, device="cuda")
    with pytest.raises(RuntimeError, match="paired image"):
        hip.gemm(a, w, torch.zeros(96, device="cuda"), epilogue=hip.EPI_BIAS_SWIGLU, out=out)
    assert bool((out == 7.0).all())                                       # an error, not a launch


def test_swiglu_epilogue_large_negative_gate_is_minus_zero():
    for tdt in (torch.bfloat16, torch.float32):
        a = torch.zeros(4, 64)
        a[:, 0] = 1.0
        w12 = torch.zeros(128, 64)
        w12[:64, 0] = -100.0
        w12[64:, 0] = 2.0
        w12p, b12p = _packed(w12, torch.zeros(128), tdt)
        for odt in (tdt, torch.float32):
            got = hip.gemm(a.to(tdt).cuda(), w12p, b12p, epilogue=hip.EPI_BIAS_SWIGLU, out_dtype=odt)
            assert bool(torch.isfinite(got).all()) and not bool(got.any())
            assert bool(torch.signbit(got).all())


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("tag,E", [("384", 384), ("128", 128)])
def test_swiglu_ffn_matches_reference_fixture(tag, E, mode):
    """SwiGLUFFNFused end to end on the device against the reference's own outputs (swiglu_ops): pack_swiglu, the w12 product with the
    SwiGLU epilogue, the w3 product on the padded image with K = Hp.  E = 128 has H = 344, padded to Hp = 384: the padded hidden columns
    meet the zero columns of w3p.  Bar: the embedding tolerance of the compute type."""
    from test_swiglu_cpu import _ffn_weights
    g = load_golden("swiglu_ops")
    seed, stream, tdt = int(g["seed"]), int(g[f"stream_{tag}"]), DT[mode]
    (w12, b12, w3, b3), H = _ffn_weights(E, seed, stream)
    x = torch.from_numpy(synth.hash_normal((int(g[f"rows_{tag}"]), E), seed, stream + 5))
    w12p, b12p, w3p = hip.pack_swiglu(w12.cuda(), b12.cuda(), w3.cuda(), tdt)
    assert w3p.shape == (E, (H + 63) // 64 * 64)
    h = hip.gemm(x.to(tdt).cuda(), w12p, b12p, epilogue=hip.EPI_BIAS_SWIGLU)
    assert h.shape == (x.shape[0], w3p.shape[1]) and h.dtype == tdt
    out = hip.gemm(h, w3p, b3.cuda(), out_dtype=torch.float32)
    err = rel_l2(out.cpu(), g[f"out_{tag}"])
    print(f"swiglu_ops {tag} {mode}: {err:.3e}")
    assert err < TOL[mode][1], err


# ---- row kernels ------------------------------------------------------------------------------------------------------------------------
def _rows_input(rows, H, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x12 = torch.randn(rows, 2 * H, device="cuda", generator=g) * 2.5
    x12[0, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0], device="cuda")    # gates at which exp(-x1) under- and overflows
    dh = torch.randn(rows, H, device="cuda", generator=g)
    return x12, dh


@pytest.mark.parametrize("rows,H", [(1, 8), (7, 344), (1030, 1024)])
def test_swiglu_rows_fp32_against_float64(rows, H):
    x12, dh = _rows_input(rows, H, rows + H)
    h, dx = hip.swiglu_fwd(x12), hip.swiglu_bwd(x12, dh)
    assert h.shape == (rows, H) and dx.shape == (rows, 2 * H)
    assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(dx).all())
    x1, x2 = x12.double().cpu().chunk(2, dim=-1)
    s = torch.sigmoid(x1)
    d = dh.double().cpu()
    assert scaled_err(h, x1 * s * x2) < 2e-5
    assert scaled_err(dx, torch.cat([d * x2 * s * (1 + x1 * (1 - s)), d * x1 * s], dim=-1)) < 2e-5
    assert float(h[0, 3]) == 0.0 and float(dx[0, 3]) == 0.0               # gate -100: sigmoid underflows to 0, nothing is NaN


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("rows,H", [(1, 8), (7, 344), (1030, 1024), (5, 7)])
def test_swiglu_rows_16bit_are_the_fp32_entry_points_on_the_upcast_input(rows, H, prec):
    """mst_swiglu_fwd16(x12) == T(mst_swiglu_fwd(float(x12))) and mst_swiglu_bwd16(x12, dh) == mst_swiglu_bwd(float(x12), dh), bit for bit;
    H = 7 takes the one-element-per-thread form."""
    T = DT[prec]
    x12, dh = _rows_input(rows, H, 3 * rows + H)
    x16 = x12.to(T)
    h16 = hip.swiglu_fwd(x16)
    assert h16.dtype == T and bool(torch.isfinite(h16.float()).all())
    assert torch.equal(_bits(h16), _bits(hip.swiglu_fwd(x16.float()).to(T)))
    dx = hip.swiglu_bwd(x16, dh)
    assert dx.dtype == torch.float32 and bool(torch.isfinite(dx).all())
    assert torch.equal(_bits(dx), _bits(hip.swiglu_bwd(x16.float(), dh)))


# ---- models -----------------------------------------------------------------------------------------------------------------------------
def _model(sd, E, depth, heads, *, ffn="swiglufused", img_size=518, layerscale=True, chunked=False, **kw):
    """A reduced-depth model: built on the meta device, the encoder replaced, materialised on the GPU, loaded strictly."""
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    with torch.device("meta"):
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, model_size={1536: "g", 1024: "l"}.get(E, "s"), ffn_layer=ffn, **kw)
        m.encoder = _ViT(E, depth, heads, img_size=img_size, layerscale=1.0 if layerscale else None, chunked=chunked, ffn_layer=ffn)
    m = m.to_empty(device="cuda")
    m.load_state_dict(sd, strict=True)
    return m


@pytest.fixture(scope="module")
def sd_s2():
    return synth.synth_state_dict("s", int(load_golden("swiglu_s2")["seed"]), img_size=518, layerscale=True, chunked=False,
                                  ffn_layer="swiglufused", depth=2)


@pytest.fixture(scope="module")
def sd_g1():
    """The one E = 1536 SwiGLU state dict of this module (its synthesis alone takes seconds): the fixture's, reused by the training tests."""
    return synth.synth_state_dict("g", int(load_golden("swiglu_g1")["seed"]), img_size=518, layerscale=True, chunked=False,
                                  ffn_layer="swiglufused", depth=1)


@pytest.fixture(scope="module")
def sd_l1():
    """One block of the ViT-L width with the GELU MLP (fc1 / fc2: 4096 x 1024, one column block more than a gridDim.y of mst_colsum),
    LayerScale and the hub layout like sd_g1.  Slices are averaged: 1024 is no multiple of the Slice Transformer's 12 heads, so the
    reference has no ViT-L with the transformer fusion either."""
    return synth.synth_state_dict("l", 71, img_size=518, layerscale=True, chunked=False, ffn_layer="mlp", depth=1, slice_fusion="average")


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_swiglu_inference_matches_reference_fixtures(mode, sd_s2):
    g = load_golden("swiglu_s2")
    tl, te, tm = TOL[mode]
    seed = int(g["seed"])
    model = _model(sd_s2, 384, 2, 6, compute_dtype=mode).eval()
    with torch.no_grad():
        for tag in ("3x28x42", "2x224x224"):                              # 21 and 514 token rows: a ragged last tile
            x = synth.synth_volume((1, 1) + tuple(int(v) for v in g[f"shape_{tag}"]), seed + 100)[0, 0]
            err = rel_l2(model.encode_slices(x.cuda().contiguous())[0].cpu(), g[f"emb_{tag}"])
            print(f"swiglu_s2 {mode} emb {tag}: {err:.3e}")
            assert err < te, (tag, err)
        src = synth.synth_volume(tuple(int(v) for v in g["model_shape"]), seed + 101)
        logits = model(src, save_attn=True)
        assert float((logits.cpu() - torch.from_numpy(g["logits"])).abs().max()) < tl
        assert len(model.attention_maps) == 2
        assert rel_l2(torch.stack([m[:, :, 0] for m in model.attention_maps]).cpu(), g["vit_cls_rows"]) < tm
        assert rel_l2(model.attention_maps_slice[-1].cpu(), g["slice_map"]) < tm
        assert rel_l2(model.get_plane_attention().cpu(), g["plane_attention"]) < tm
        assert rel_l2(model.get_slice_attention().cpu(), g["slice_attention"]) < tm
        assert rel_l2(model.get_attention_maps().cpu(), g["attention_maps"]) < tm
        assert torch.equal(model(src), logits)
        # prune_last_block: the last block's FFN on the CLS rows alone
        pruned = _model(sd_s2, 384, 2, 6, compute_dtype=mode, prune_last_block=True).eval()
        assert float((pruned(src) - logits).abs().max()) < tl
        assert float((pruned(src).cpu() - torch.from_numpy(g["logits"])).abs().max()) < tl
        # the chunked key layout loads into the unchunked encoder and the other way round
        chunked = {k.replace("encoder.blocks.", "encoder.blocks.0."): v for k, v in sd_s2.items()}
        assert torch.equal(_model(chunked, 384, 2, 6, compute_dtype=mode).eval()(src), logits)
        assert torch.equal(_model(sd_s2, 384, 2, 6, compute_dtype=mode, chunked=True).eval()(src), logits)


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_swiglu_g_width_inference_matches_reference_fixture(mode, sd_g1):
    g = load_golden("swiglu_g1")
    model = _model(sd_g1, 1536, 1, 24, compute_dtype=mode).eval()
    x = synth.synth_volume((1, 1) + tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)[0, 0]
    with torch.no_grad():
        err = rel_l2(model.encode_slices(x.cuda().contiguous())[0].cpu(), g["emb"])
    print(f"swiglu_g1 {mode} emb: {err:.3e}")
    assert err < TOL[mode][1], err


@pytest.mark.parametrize("mode", ["fp32", "fp16", "bf16"])
def test_g_width_with_the_plain_mlp_matches_the_oracle(mode, monkeypatch):
    """model_size='g' as pretrained=False builds it (GELU MLP, chunked layout), one block: E = 1536 and 24 heads through every stage --
    tokens, attention, MLP, the slice transformer at head_dim 128, the attention read-outs -- with a key-padding mask."""
    from oracle import mst_oracle as O
    monkeypatch.setitem(O.VIT_CFG, "g1", dict(embed_dim=1536, depth=1, num_heads=24))
    tl, te, tm = TOL[mode]
    sd = synth.synth_state_dict("g", 61, depth=1)
    src = synth.synth_volume((2, 1, 3, 56, 70), 161)
    mask = torch.zeros(2, 3, dtype=torch.bool)
    mask[1, 2] = True
    with torch.no_grad():
        ref = O.forward(sd, src, model_size="g1", src_key_padding_mask=mask, keep="cls")
    model = _model(sd, 1536, 1, 24, ffn="mlp", img_size=224, layerscale=False, chunked=True, compute_dtype=mode).eval()
    with torch.no_grad():
        logits = model(src, save_attn=True, src_key_padding_mask=mask)
        emb = model.encode_slices(src.cuda().reshape(6, 56, 70))[0]
    errs = (float((logits.cpu() - ref["logits"]).abs().max()), rel_l2(emb.cpu(), ref["emb"]))
    print(f"g width, MLP, {mode}: logits {errs[0]:.3e} emb {errs[1]:.3e}")
    assert errs[0] < tl and errs[1] < te, errs
    assert rel_l2(torch.stack([m[:, :, 0] for m in model.attention_maps]).cpu(), torch.stack([m[:, :, 0] for m in ref["vit_maps"]])) < tm
    assert rel_l2(model.attention_maps_slice[-1].cpu(), ref["slice_map"]) < tm
    assert rel_l2(model.get_plane_attention().cpu(), O.plane_attention(ref["vit_maps"][-1])) < tm
    assert rel_l2(model.get_attention_maps().cpu(), O.attention_maps(ref["vit_maps"][-1], ref["slice_map"])) < tm


def test_g_width_deep_volume_matches_the_oracle(monkeypatch):
    """The same one-block g model on a 200-slice volume with its last 60 slices masked: the slice transformer at head_dim 128 with 201
    tokens, more than K and V of a head fill in LDS (159 tokens), so the attention reads V from global memory (csrc/k_slice.hip).
    One 14 x 14 patch per slice keeps the encoder small; one state dict and one oracle run serve the three compute types."""
    from oracle import mst_oracle as O
    monkeypatch.setitem(O.VIT_CFG, "g1", dict(embed_dim=1536, depth=1, num_heads=24))
    sd = synth.synth_state_dict("g", 61, depth=1)
    src = synth.synth_volume((1, 1, 200, 14, 14), 162)
    mask = torch.zeros(1, 200, dtype=torch.bool)
    mask[0, 140:] = True
    with torch.no_grad():
        ref = O.forward(sd, src, model_size="g1", src_key_padding_mask=mask, keep="cls")
    for mode in ("fp32", "fp16", "bf16"):
        tl, te, tm = TOL[mode]
        model = _model(sd, 1536, 1, 24, ffn="mlp", img_size=224, layerscale=False, chunked=True, compute_dtype=mode).eval()
        with torch.no_grad():
            logits = model(src, save_attn=True, src_key_padding_mask=mask)
        err, merr = float((logits.cpu() - ref["logits"]).abs().max()), rel_l2(model.attention_maps_slice[-1].cpu(), ref["slice_map"])
        print(f"g width, 200 slices, {mode}: logits {err:.3e} slice map {merr:.3e}")
        assert err < tl and merr < tm, (mode, err, merr)
        assert torch.equal(model.attention_maps_slice[-1][0, :, :, 141:].cpu(), torch.zeros(12, 201, 60))


# ---- training ---------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _deterministic(on):
    prev, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn)


def _step(model, src, target, mask=None):
    model.zero_grad(set_to_none=True)
    source = src.cuda().requires_grad_()
    logits = model(source, src_key_padding_mask=mask)
    F.cross_entropy(logits, target.cuda()).backward()
    grads = {k: p.grad for k, p in model.named_parameters()}
    grads[P.SOURCE] = source.grad
    return logits.detach(), grads


_REF = {}


def _float64_grads(name, sd, src, depth, heads, target, **kw):
    if name not in _REF:                                                  # computed once, shared by the atomic and the ordered run
        _REF[name] = R.grads(sd, src, depth, heads, target, **kw)
    return _REF[name]


@pytest.mark.parametrize("det", [False, True], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("case", ["s2_layerscale", "g1", "g1_m136", "l1"])
def test_fp32_step_matches_float64_autograd(case, det, sd_s2, sd_g1, sd_l1):
    """Every parameter gradient and d source of the fp32 step against float64 autograd through tests/swiglu_ref.py, at the bar of
    tests/train_parity.py (1e-4 of max |ref| + 1e-9: its derivation -- the reference's own fp32 noise -- applies unchanged); under
    torch.use_deterministic_algorithms(True) two steps give the same bits.  g1 has 34 token rows: every weight gradient is one product.
    g1_m136 and l1 (E = 1024, 16 heads, the GELU MLP) have 8 x 17 = 136: `_dw` splits them in two and reduces [2, N K] partials of 4.2 M
    (fc1 / fc2 of l1) to 12.6 M columns (w12 of g1) with mst_colsum -- atomic with the flag off, ordered with it on."""
    sd, E, depth, heads, shape, ffn, fusion = {"s2_layerscale": (sd_s2, 384, 2, 6, (2, 1, 3, 70, 56), "swiglufused", "transformer"),
                                               "g1": (sd_g1, 1536, 1, 24, (1, 1, 2, 56, 56), "swiglufused", "transformer"),
                                               "g1_m136": (sd_g1, 1536, 1, 24, (1, 1, 8, 56, 56), "swiglufused", "transformer"),
                                               "l1": (sd_l1, 1024, 1, 16, (1, 1, 8, 56, 56), "mlp", "average")}[case]
    src, target = synth.synth_volume(shape, 171), torch.arange(shape[0]) % 2
    _, logits_ref, ref = _float64_grads(case, sd, src, depth, heads, target, slice_fusion_type=fusion)
    with _deterministic(det):
        model = _model(sd, E, depth, heads, ffn=ffn, slice_fusion=fusion, compute_dtype="fp32").train()
        logits, got = _step(model, src, target)
        errs = P.scaled_errors(got, ref)
        worst = max(errs, key=errs.get)
        print(f"{case} deterministic={det}: worst scaled gradient error {errs[worst]:.3e} ({worst}), source {errs[P.SOURCE]:.3e}, "
              f"logits {float((logits.cpu().double() - logits_ref).abs().max()):.3e}")
        assert float((logits.cpu().double() - logits_ref).abs().max()) < TOL["fp32"][0]
        P.check(got, ref)
        if det:
            got = {k: (None if g is None else g.clone()) for k, g in got.items()}
            logits2, again = _step(model, src, target)
            assert torch.equal(logits2, logits)
            for k, g in got.items():
                assert (g is None and again[k] is None) or torch.equal(g, again[k]), k


SHAPE16 = (1, 1, 4, 224, 224)


@pytest.fixture(scope="module")
def fp32_step(sd_s2):
    src, tgt = synth.synth_volume(SHAPE16, 3), torch.tensor([1])
    logits, grads = _step(_model(sd_s2, 384, 2, 6).train(), src, tgt)
    return logits, {k: g.clone() for k, g in grads.items() if g is not None and k != P.SOURCE}


@pytest.mark.parametrize("storage", ["fp32", "16bit"])
@pytest.mark.parametrize("prec,bars", [("fp16", (1e-2, 8e-3)), ("bf16", (1.3e-1, 7e-2))])
def test_16bit_steps_against_the_fp32_step(prec, bars, storage, sd_s2, fp32_step):
    """train_precision fp16 / bf16 with train_attention='flash', fp32 and 16-bit storage, at E = 384 depth 2 with LayerScale and
    (1, 1, 4, 224, 224), against this build's own fp32 step (held to float64 by the test above): logits and every parameter gradient inside
    the bars of tests/test_train_storage_gpu.py -- fp16 1e-2 per parameter / 8e-3 global rel-L2, bf16 1.3e-1 / 7e-2.  The arithmetic alone
    (tests/test_swiglu_cpu.py, float64 with the kernels' roundings) gives at most 1.1e-3 / 3.0e-3 / 2.6e-3 (fp16) and 2.1e-2 / 3.7e-2 /
    3.1e-2 (bf16) for logits / worst parameter / global, so the bars stand as they are."""
    src, tgt = synth.synth_volume(SHAPE16, 3), torch.tensor([1])
    model = _model(sd_s2, 384, 2, 6, train_precision=prec, train_attention="flash", train_storage=storage).train()
    logits, grads = _step(model, src, tgt)
    got = (logits, {k: g for k, g in grads.items() if g is not None and k != P.SOURCE})
    assert all(bool(torch.isfinite(g).all()) for g in got[1].values())
    d, w, g = _compare(got, fp32_step)
    print(f"swiglu {prec} storage={storage} vs fp32: logits {d:.2e} worst {w:.2e} global {g:.2e}")
    assert d < bars[0] and w < bars[0] and g < bars[1], (d, w, g)


def test_stored_attention_mixed_precision_step_runs(sd_s2, fp32_step):
    """train_precision='fp16' with train_attention='stored' (fp32 storage): the third combination of the mode table, at the fp16 bars."""
    src, tgt = synth.synth_volume(SHAPE16, 3), torch.tensor([1])
    logits, grads = _step(_model(sd_s2, 384, 2, 6, train_precision="fp16", train_attention="stored").train(), src, tgt)
    d, w, g = _compare((logits, {k: v for k, v in grads.items() if v is not None and k != P.SOURCE}), fp32_step)
    assert d < 1e-2 and w < 1e-2 and g < 8e-3, (d, w, g)


def test_frozen_model_source_gradient_is_the_trainable_model_s(sd_s2):
    src, tgt = synth.synth_volume((2, 1, 3, 70, 56), 171), torch.tensor([0, 1])
    model = _model(sd_s2, 384, 2, 6).train()
    _, grads = _step(model, src, tgt)
    model.requires_grad_(False)
    frozen = src.cuda().requires_grad_()
    F.cross_entropy(model(frozen), tgt.cuda()).backward()
    assert frozen.grad is not None and bool(torch.isfinite(frozen.grad).all())
    assert rel_l2(frozen.grad.cpu(), grads[P.SOURCE].cpu()) < 1e-6
