"""Gradients with respect to the input volume of DinoV2ClassifierSlice: ``source.grad`` / ``torch.autograd.grad(logits, source)``, what the
reference's plain-torch forward gives for free (gradient saliency, attribution, adversarial checks).  The patch embedding's data gradient
(mst_patch_embed_dgrad, csrc/k_patch_dgrad.hip) against fp64 autograd of the reference's conv; whole-model source gradients against
float64 torch.autograd through the CPU oracle at the parameter bar (1e-4 * max |ref|, tests/train_parity.py), with every parameter gradient
of the same backward still at that bar; input dtypes / devices / channels; frozen models; the mixed-precision steps; bit-reproducibility
under the determinism flag."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_l2
from mst import hip, synth
from test_model_gpu import CASES, build

pytestmark = pytest.mark.gpu


def _wsum(w: torch.Tensor) -> torch.Tensor:
    """[E, 3, 14, 14] conv weight -> the [E, 14 * 16] channel sum the forward's mst_patch_embed reads (columns 14, 15 zero)."""
    ws = torch.zeros(w.shape[0], 14, 16, dtype=torch.float32)
    ws[:, :, :14] = w.float().sum(1)
    return ws.view(w.shape[0], 224)


@pytest.mark.parametrize("E,n,H,W,R", [(384, 3, 56, 56, 0), (768, 5, 112, 140, 0), (1024, 2, 70, 42, 4), (384, 7, 42, 98, 1)])
def test_patch_embed_dgrad_matches_fp64_autograd_of_the_conv(E, n, H, W, R):
    """n * Np is never a multiple of the 64-row tile; H != W; with R > 0 the patch rows are read straight out of the encoder's token
    gradient (row s * (1 + R + Np) + 1 + R + p).  Every pixel is written (the output starts as NaN)."""
    g = torch.Generator().manual_seed(E + n)
    gh, gw = H // 14, W // 14
    Np = gh * gw
    w = torch.randn(E, 3, 14, 14, generator=g, dtype=torch.float64) * 0.05
    dpatch = torch.randn(n * Np, E, generator=g, dtype=torch.float64)
    x = torch.zeros(n, 1, H, W, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.repeat(1, 3, 1, 1), w, stride=14)                                  # [n, E, gh, gw]
    ref, = torch.autograd.grad(y, x, dpatch.view(n, gh, gw, E).permute(0, 3, 1, 2))
    ref = ref[:, 0]
    N = 1 + R + Np
    dx = torch.randn(n, N, E, generator=g, dtype=torch.float64)                        # prefix rows hold noise the kernel must not read
    dx[:, 1 + R:] = dpatch.view(n, Np, E)
    out = torch.full((n, H, W), float("nan"), dtype=torch.float32, device="cuda")
    got = hip.patch_embed_dgrad(dx.float().cuda().view(n * N, E), _wsum(w).cuda(), n, H, W, tokens=N, first=1 + R, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    got = got.cpu().double()
    assert bool(torch.isfinite(got).all()), "pixels left unwritten"
    err = float((got - ref).abs().max())
    assert err <= 1e-5 * float(ref.abs().max()), err
    if R == 0:                                          # the plain [n * Np, E] form gives the same bits
        again = hip.patch_embed_dgrad(dpatch.float().cuda(), _wsum(w).cuda(), n, H, W)
        assert torch.equal(again.cpu().double(), got)


def _sd(kw, seed):
    return synth.synth_state_dict(kw.get("model_size", "s"), seed, use_bottleneck=kw.get("use_bottleneck", False),
                                  use_slice_pos_emb=kw.get("use_slice_pos_emb", False),
                                  slice_fusion=kw.get("slice_fusion", "transformer"), rotary=kw.get("rotary_positional_encoding"))


def _oracle(sd, kw, src, mask, target, params=True, loss="ce"):
    """float64 torch.autograd through the CPU oracle: (d source, {name: d parameter} or None)."""
    from oracle import mst_oracle as O
    sd = {k: (v.double().requires_grad_(params and not k.endswith("rotary_positional_encoding.freqs")) if v.is_floating_point() else v.clone())
          for k, v in sd.items()}
    x = src.detach().double().requires_grad_(True)
    y = O.forward(sd, x, model_size=kw.get("model_size", "s"), slice_fusion_type=kw.get("slice_fusion", "transformer"),
                  src_key_padding_mask=mask, rotary=kw.get("rotary_positional_encoding"))["logits"]
    (F.cross_entropy(y, target) if loss == "ce" else y[:, 1].sum()).backward()
    return x.grad, ({k: v.grad for k, v in sd.items()} if params else None)


RTOL = 1e-4
# max |d - ref| / max |ref| against the float64 oracle, measured on the MI355X (source gradient / worst parameter)
MEASURED = {
    "c1_1x16x224": (3.1e-6, 8.1e-6), "b2_mask": (9.6e-6, 1.2e-5), "bottleneck_pos": (8.9e-6, 9.2e-6), "rope": (1.2e-5, 1.1e-5),
    "average": (8.9e-6, 7.8e-6), "registers": (5.8e-6, 1.3e-5), "channels": (1.3e-5, 1.2e-5), "fp16": (2.4e-6, 1.6e-5),
    "bf16": (8.5e-7, 1.2e-5), "cpu": (5.2e-6, 1.1e-5), "frozen eval": (7.4e-6, None), "freeze=True": (9.6e-6, 8.2e-6),
}   # all <= 3e-5: every case is held to RTOL


def _close(got, ref, rtol=RTOL, extra=0.0):
    got = got.detach().cpu().double()
    ref = ref.double()
    assert got.shape == ref.shape
    scale = float(ref.abs().max())
    assert scale > 0
    err = float(((got - ref).abs() - extra * ref.abs()).max())
    assert err <= rtol * scale + 1e-9, (err, scale)
    return err / scale


def _check_params(model, ref, label=""):
    worst = {}
    for k, p in model.named_parameters():
        r = ref.get(k)
        if r is None:                                   # unused by the forward (mask_token)
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        worst[k] = _close(p.grad, r)
    print(label, "worst relative parameter-gradient error:", max(worst.values()), max(worst, key=worst.get))


@pytest.mark.parametrize("name", ["c1_1x16x224", "b2_mask", "bottleneck_pos", "rope", "average"])
def test_source_gradient_and_every_parameter_gradient_match_oracle_autograd(name):
    g = load_golden(name)
    kw = CASES[name]
    seed = int(g["seed"])
    model = build(kw, seed, "fp32").train()
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), seed + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"]) if "src_key_padding_mask" in g else None
    target = torch.arange(src.shape[0]) % 2
    ref_src, ref = _oracle(_sd(kw, seed), kw, src, mask, target)
    source = src.cuda().requires_grad_(True)
    F.cross_entropy(model(source, src_key_padding_mask=mask), target.cuda()).backward()
    assert source.grad is not None and source.grad.dtype == torch.float32 and source.grad.is_cuda
    print(name, "source gradient relative error:", _close(source.grad, ref_src))
    _check_params(model, ref, name)


def test_register_token_encoder_source_gradient_at_the_stored_grid():
    from oracle import mst_oracle as O
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    seed = 23
    sd = synth.synth_state_dict("s", seed, img_size=56, layerscale=True, chunked=False, num_register_tokens=4)
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_registers=True)
    model.encoder = _ViT(384, 12, 6, img_size=56, num_register_tokens=4, layerscale=1.0, chunked=False)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    src = synth.synth_volume((2, 1, 3, 56, 56), seed + 100)
    target = torch.tensor([1, 0])
    sdg = {k: v.double().requires_grad_() for k, v in sd.items()}
    x = src.double().requires_grad_(True)
    F.cross_entropy(O.forward(sdg, x)["logits"], target).backward()
    source = src.cuda().requires_grad_(True)
    F.cross_entropy(model(source), target.cuda()).backward()
    print("registers source gradient relative error:", _close(source.grad, x.grad))
    _check_params(model, {k: v.grad for k, v in sdg.items()}, "registers")


@pytest.mark.parametrize("form", ["channels", "fp16", "bf16", "cpu"])
def test_source_forms_give_a_gradient_of_the_same_shape_dtype_and_device(form):
    """C > 1 (channels become slices, channel fastest: dino.py:125), 16-bit sources, a source on the host."""
    seed = 5
    shape = (1, 3, 2, 56, 56) if form == "channels" else (2, 1, 3, 56, 42)
    src = synth.synth_volume(shape, seed + 100)
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(form, torch.float32)
    src = src.to(dtype)
    source = (src if form == "cpu" else src.cuda()).requires_grad_(True)
    model = build({}, seed, "fp32").train()
    target = torch.tensor([1, 0][:shape[0]])
    F.cross_entropy(model(source), target.cuda()).backward()
    ref_src, ref = _oracle(_sd({}, seed), {}, src.float(), None, target)
    gs = source.grad
    assert gs is not None and gs.shape == source.shape and gs.dtype == source.dtype and gs.device == source.device
    # the gradient is computed in fp32 and rounded to the source's type once
    print(form, "source gradient relative error:", _close(gs.float(), ref_src, extra={torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}.get(dtype, 0.0)))
    _check_params(model, ref, form)


def test_frozen_model_source_gradient_routes_to_the_training_step():
    """All parameters frozen, .eval(): the logits carry the autograd node only because the source requires grad; no parameter gets a .grad."""
    g = load_golden("b2_mask")
    seed = int(g["seed"])
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), seed + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"])
    model = build({}, seed, "fp32").eval()
    model.requires_grad_(False)
    source = src.cuda().requires_grad_(True)
    logits = model(source, src_key_padding_mask=mask)
    assert logits.grad_fn is not None
    d, = torch.autograd.grad(logits[:, 1].sum(), source)
    ref_src, _ = _oracle(_sd({}, seed), {}, src, mask, None, params=False, loss="logit1")
    print("frozen eval source gradient relative error:", _close(d, ref_src))
    assert all(p.grad is None for p in model.parameters())
    # the logits are the reference forward's too
    assert float((logits.detach().cpu() - torch.from_numpy(g["logits"])).abs().max()) < 1e-4
    with torch.no_grad():                               # no-grad calls stay on the inference path
        assert model(source, src_key_padding_mask=mask).grad_fn is None


def test_freeze_encoder_with_a_source_gradient():
    """freeze=True (dino.py:65-67): the encoder's parameters get no gradient, the rest are as before, and d source runs through the frozen
    encoder's d x chain."""
    from mst.models import DinoV2ClassifierSlice
    g = load_golden("b2_mask")
    seed = int(g["seed"])
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), seed + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"])
    fm = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", freeze=True)
    fm.load_state_dict(_sd({}, seed))
    fm = fm.cuda().train()
    target = torch.tensor([0, 1])
    ref_src, ref = _oracle(_sd({}, seed), {}, src, mask, target)
    source = src.cuda().requires_grad_(True)
    F.cross_entropy(fm(source, src_key_padding_mask=mask), target.cuda()).backward()
    worst = 0.0
    for k, p in fm.named_parameters():
        if k.startswith("encoder."):
            assert p.grad is None, k
        else:
            worst = max(worst, _close(p.grad, ref[k]))
    print("freeze=True: source gradient relative error", _close(source.grad, ref_src), "worst parameter", worst)


def _step_src_grad(prec, attn, src, tgt):
    from mst.models import DinoV2ClassifierSlice
    m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, train_precision=prec, train_attention=attn)
    m.load_state_dict(synth.synth_state_dict("s", 0))
    m = m.cuda().train()
    source = src.clone().requires_grad_(True)
    F.cross_entropy(m(source), tgt).backward()
    return source.grad


# relative L2 of the 16-bit steps' source gradient against the fp32 step's.  Measured on the MI355X (stored / flash): fp16 5.3e-3 / 5.8e-3,
# bf16 3.9e-2 / 3.6e-2; 2x that is looser than the mixed-precision step's parameter bars, so those bars hold here
MIXED_BAR = {"fp16": 8e-3, "bf16": 7e-2}


@pytest.mark.parametrize("attn", ["stored", "flash"])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_mixed_precision_source_gradient_against_the_fp32_step(prec, attn):
    src = synth.synth_volume((1, 1, 4, 224, 224), 3).cuda()
    tgt = torch.tensor([1]).cuda()
    g32 = _step_src_grad("fp32", "stored", src, tgt)
    g16 = _step_src_grad(prec, attn, src, tgt)
    err = rel_l2(g16.cpu(), g32.cpu())
    print(f"source gradient {prec} {attn}: relative L2 {err:.3e}")
    assert err < MIXED_BAR[prec], err


def test_source_gradient_is_bit_reproducible_under_the_determinism_flag():
    g = load_golden("b2_mask")
    seed = int(g["seed"])
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), seed + 100).cuda()
    mask = torch.from_numpy(g["src_key_padding_mask"])
    model = build({}, seed, "fp32").train()
    target = torch.tensor([0, 1]).cuda()
    prev, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        runs = []
        for _ in range(2):
            source = src.clone().requires_grad_(True)
            model.zero_grad(set_to_none=True)
            F.cross_entropy(model(source, src_key_padding_mask=mask), target).backward()
            runs.append((source.grad.clone(), model.encoder.patch_embed.proj.weight.grad.clone()))
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn)
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
