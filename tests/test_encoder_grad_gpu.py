"""Gradients through the encoder API on the device (``encoder_grad=True``): the three op-level entries of the RGB patch embedding against
float64 F.conv2d and its autograd, every case of tests/encoder_grad_ref.py against float64 autograd through the restatement at the bar the
CPU test derives from the reference alone, and what the switch must leave alone."""
import pytest
import torch
import torch.nn.functional as F

import encoder_grad_ref as EG
from conftest import rel_l2
from mst import hip, synth
from test_model_gpu import TOL

pytestmark = pytest.mark.gpu

OP_BAR = 1e-5            # tests/test_input_grad_gpu.py holds mst_patch_embed_dgrad to 1e-5 * max |ref|: exact fp32 MFMA, E-term sums
GUARD = 256              # floats on either side of an output


def _normal(shape, seed, std=1.0):
    return torch.from_numpy(synth.hash_normal(tuple(shape), seed)).double() * std


def _guarded(shape):
    """A contiguous fp32 tensor of `shape` inside a buffer filled with a sentinel, and the check that the band around it still holds it."""
    numel = int(torch.Size(shape).numel())
    buf = torch.full((numel + 2 * GUARD,), -77.0, dtype=torch.float32, device="cuda")

    def untouched():
        return bool((buf[:GUARD] == -77.0).all()) and bool((buf[GUARD + numel:] == -77.0).all())
    return buf[GUARD:GUARD + numel].view(shape), untouched


def _close(got, ref, bar):
    err = float((got.detach().cpu().double() - ref).abs().max())
    assert err <= bar * float(ref.abs().max()), (err, float(ref.abs().max()))
    return err / float(ref.abs().max())


# ---- 1. op level -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [384, 768])
@pytest.mark.parametrize("shape", [(2, 3, 56, 70), (3, 3, 70, 84)])
def test_rgb_patch_embedding_ops_against_fp64_conv2d_and_its_autograd(shape, E):
    n, _, H, W = shape
    gh, gw = H // 14, W // 14
    Np, R = gh * gw, 2
    N = 1 + R + Np
    img = _normal(shape, 1).requires_grad_()
    w = _normal((E, 3, 14, 14), 2, 0.05).requires_grad_()
    bias, prefix, pos = _normal((E,), 3), _normal((1 + R, E), 4), _normal((Np, E), 5)
    ref = F.conv2d(img, w, bias, stride=14).flatten(2).transpose(1, 2) + pos            # [n, Np, E]
    dx = _normal((n, N, E), 6)                                                           # prefix rows carry a gradient too: it must not leak
    (ref * dx[:, 1 + R:]).sum().backward()
    wp = hip.pack_patch_rgb(w.detach().float().cuda(), torch.float32)
    imgd, dxd = img.detach().float().cuda(), dx.float().cuda().view(n * N, E)
    # forward
    x = hip.patch_embed_rgb(imgd, wp, bias.float().cuda(), prefix.float().cuda(), pos.float().cuda())
    assert tuple(x.shape) == (n, N, E) and torch.equal(x[:, :1 + R].cpu(), prefix.float().expand(n, -1, -1))
    e_fwd = _close(x[:, 1 + R:], ref.detach(), OP_BAR)
    # input gradient: every pixel written once, nothing beyond, the same bits run to run (flag off: there is no reduction to order)
    assert not torch.are_deterministic_algorithms_enabled()
    dimg, untouched = _guarded(shape)
    hip.patch_embed_rgb_dgrad(dxd, wp, n, H, W, tokens=N, first=1 + R, out=dimg)
    e_dgrad = _close(dimg, img.grad, OP_BAR)
    assert untouched()
    assert torch.equal(hip.patch_embed_rgb_dgrad(dxd, wp, n, H, W, tokens=N, first=1 + R), dimg)
    wsum = torch.zeros(E, 14, 16)
    wsum[..., :14] = w.detach().sum(1).float()
    grey = hip.patch_embed_dgrad(dxd, wsum.view(E, 224).cuda(), n, H, W, tokens=N, first=1 + R)
    _close(dimg.sum(1), grey.cpu().double(), OP_BAR)
    # weight gradient
    splits = -(-n * Np // hip.rgb_wgrad_split_rows(n * Np))
    part, untouched = _guarded((splits, E * 588))
    dW = hip.patch_embed_rgb_wgrad(dxd, imgd, E, tokens=N, first=1 + R, part=part)
    assert tuple(dW.shape) == (E, 3, 14, 14) and untouched()
    e_wgrad = _close(dW, w.grad, EG.BAR)
    # three equal channels: three bit-equal planes of dW
    eq = imgd[:, :1].expand(n, 3, H, W).contiguous()
    dWe = hip.patch_embed_rgb_wgrad(dxd, eq, E, tokens=N, first=1 + R)
    assert torch.equal(dWe[:, 0], dWe[:, 1]) and torch.equal(dWe[:, 0], dWe[:, 2])
    print(f"{shape} E={E}: forward {e_fwd:.2e}, dgrad {e_dgrad:.2e} (bar {OP_BAR:g}), wgrad {e_wgrad:.2e} (bar {EG.BAR:g})")


@pytest.mark.parametrize("shape,splits", [((2, 3, 140, 196), 2), ((5, 3, 406, 420), 16)])
def test_rgb_weight_gradient_over_several_partials(shape, splits):
    """280 patch rows: two partials of 256 rows, the second ragged.  4350 rows: beyond 16 x 256 the split grows to 272 rows, 16 partials,
    the last of 270 rows (16 whole K-steps and 14 rows of one)."""
    n, _, H, W = shape
    E, Np = 384, (H // 14) * (W // 14)
    assert -(-n * Np // hip.rgb_wgrad_split_rows(n * Np)) == splits and (n * Np) % hip.rgb_wgrad_split_rows(n * Np) != 0
    img, w = _normal(shape, 11), _normal((E, 3, 14, 14), 12, 0.05).requires_grad_()
    dx = _normal((n, Np, E), 13)
    (F.conv2d(img, w, None, stride=14).flatten(2).transpose(1, 2) * dx).sum().backward()
    part, untouched = _guarded((splits, E * 588))
    for det in (False, True):
        with (EG.deterministic() if det else torch.enable_grad()):
            dW = hip.patch_embed_rgb_wgrad(dx.float().cuda().view(n * Np, E), img.float().cuda(), E, part=part)
        print(f"{shape}: {splits} partials, deterministic={det}: {_close(dW, w.grad, EG.BAR):.2e} (bar {EG.BAR:g})")
    assert untouched()


# ---- 2. every case, fp32 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(EG.CASES))
def test_every_output_and_gradient_of_the_case_against_fp64_autograd(case):
    loss_ref, outs_ref, ref = EG.ref_grads(case)
    model = EG.build_model(case)
    loss, outs, got = EG.device_grads(model, case)
    assert [k for k, _ in outs] == [k for k, _ in outs_ref]
    for (k, o), (_, r) in zip(outs, outs_ref):
        assert o.dtype == torch.float32 and o.is_cuda and tuple(o.shape) == tuple(r.shape), k
        assert rel_l2(o.cpu(), r) < TOL["fp32"][1], (k, rel_l2(o.cpu(), r))
    assert abs(loss - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref))
    assert tuple(got[EG.SOURCE].shape) == EG.CASES[case][1]
    errs = EG.scaled_errors(got, ref)
    worst = max(errs, key=errs.get)
    print(f"{case}: worst scaled error {errs[worst]:.2e} ({worst}), x.grad {errs[EG.SOURCE]:.2e}; bar {EG.BAR:g}")
    EG.check(got, ref)
    if case == "grey_28x42":                             # one grey plane: the weight gradient is the same over the three channels
        dW = got["encoder.patch_embed.proj.weight"]
        assert torch.equal(dW[:, 0], dW[:, 1]) and torch.equal(dW[:, 0], dW[:, 2])
    if case == "tap3_only":                              # blocks 4 .. 11 and encoder.norm are not walked
        assert got["encoder.norm.weight"] is None and got["encoder.blocks.0.4.norm1.weight"] is None
        assert got["encoder.blocks.0.11.mlp.fc2.weight"] is None and got["encoder.blocks.0.3.mlp.fc2.weight"] is not None


# ---- 3. a frozen encoder under an input that requires grad ----------------------------------------------------------------------------
def test_frozen_encoder_gives_the_input_gradient_alone():
    case = "rgb_56x70"
    _, _, ref = EG.ref_grads(case)
    model = EG.build_model(case)
    for p in model.parameters():
        p.requires_grad_(False)
    _, _, got = EG.device_grads(model, case)
    assert all(p.grad is None for p in model.parameters())
    errs = EG.check({EG.SOURCE: got[EG.SOURCE]}, {EG.SOURCE: ref[EG.SOURCE]})
    print(f"frozen encoder: x.grad {errs[EG.SOURCE]:.2e}")
    x = EG.image(case).cuda().requires_grad_()
    out = model.encoder.forward_features(x)["x_norm_patchtokens"]
    (g,) = torch.autograd.grad(out.square().sum(), x)
    assert tuple(g.shape) == tuple(x.shape) and bool(g.isfinite().all()) and bool(g.any()) and x.grad is None


# ---- 4. the mixed modes against the fp32 run of the same call ---------------------------------------------------------------------------
def _classifier_bars():
    import test_train_gpu
    mark = next(m for m in test_train_gpu.test_mixed_precision_step_gradients_against_the_fp32_step.pytestmark if m.name == "parametrize")
    return {prec: (bar, gbar) for prec, bar, gbar in mark.args[1]}


@pytest.mark.parametrize("prec,extra", [("fp16", {}), ("bf16", dict(train_attention="flash", train_storage="16bit"))])
def test_mixed_modes_against_the_fp32_run(prec, extra):
    """The bars of the classifier's mixed-precision test (relative L2 per tensor and over all together), x.grad counted as one more tensor.
    [2, 3, 56, 224]: 2 x 65 tokens (heights are multiples of 14), enough rows for the 16-bit products to engage."""
    bar, gbar = _classifier_bars()[prec]
    x0 = EG.ER.rgb_image((2, 3, 56, 224), 5)

    def grads(**kw):
        model = EG.build_model("rgb_56x70", **kw)
        _, outs, g = EG.device_grads(model, "rgb_56x70", x0)
        return outs, {k: v for k, v in g.items() if v is not None}
    o32, g32 = grads()
    o16, g16 = grads(train_precision=prec, **extra)
    assert set(g16) == set(g32)
    for (k, a), (_, b) in zip(o16, o32):
        assert rel_l2(a.cpu(), b.cpu()) < bar, (k, rel_l2(a.cpu(), b.cpu()))
    rel = {k: float((g16[k] - g32[k]).norm() / g32[k].norm().clamp_min(1e-30)) for k in g32}
    worst = max(rel, key=rel.get)
    glob = (sum(float((g16[k] - g32[k]).square().sum()) for k in g32) / sum(float(g32[k].square().sum()) for k in g32)) ** 0.5
    print(f"{prec} {extra}: worst tensor {rel[worst]:.3e} ({worst}; bar {bar:g}), all together {glob:.3e} (bar {gbar:g}), x.grad {rel[EG.SOURCE]:.3e}")
    assert rel[worst] < bar, (worst, rel[worst])
    assert glob < gbar, glob


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------------
def test_two_backward_passes_are_bit_identical_under_the_deterministic_flag():
    model = EG.build_model("rgb_56x70")
    with EG.deterministic():
        l1, o1, g1 = EG.device_grads(model, "rgb_56x70")
        g1 = {k: (v.clone() if v is not None else None) for k, v in g1.items()}
        l2, o2, g2 = EG.device_grads(model, "rgb_56x70")
    assert l1 == l2 and all(torch.equal(a, b) for (_, a), (_, b) in zip(o1, o2))
    assert g1["encoder.patch_embed.proj.weight"] is not None
    for k, v in g1.items():
        assert (v is None and g2[k] is None) or torch.equal(v, g2[k]), k


# ---- 6. default and state ------------------------------------------------------------------------------------------------------------------
def _calls(enc, x):
    return (lambda: enc(x), lambda: enc.forward_features(x), lambda: enc.get_intermediate_layers(x, n=[0, 5, 11], reshape=True))


def _tensors(res):
    if isinstance(res, dict):
        return [v for v in res.values() if torch.is_tensor(v)]
    return [t for r in (res if isinstance(res, tuple) else (res,)) for t in (r if isinstance(r, tuple) else (r,))]


def test_the_switch_is_off_by_default_and_no_grad_calls_keep_nothing():
    x = EG.image("rgb_56x70").cuda()
    off = EG.build_model("rgb_56x70", encoder_grad=False)
    assert torch.is_grad_enabled() and any(p.requires_grad for p in off.encoder.parameters())
    for call in _calls(off.encoder, x):
        with pytest.raises(NotImplementedError, match="no_grad"):
            call()
    on = EG.build_model("rgb_56x70")
    with torch.no_grad():
        for c_on, c_off in zip(_calls(on.encoder, x), _calls(off.encoder, x)):
            want = _tensors(c_off())
            c_on()                                       # the first call builds the model's weight images and workspaces
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            res = c_on()
            got = _tensors(res)
            after = torch.cuda.memory_allocated()
            assert len(got) == len(want) and all(torch.equal(a, b) and not a.requires_grad for a, b in zip(got, want))
            stores = {t.untyped_storage().data_ptr(): t.untyped_storage().nbytes() for t in got if t.numel()}
            assert after - before == sum(-(-b // 512) * 512 for b in stores.values()), (after - before, stores)
            del res, got
            assert torch.cuda.memory_allocated() == before
    on.encoder_grad = False                              # read at every call
    with pytest.raises(NotImplementedError, match="no_grad"):
        on.encoder(x)


# ---- 7. the classifier's step is unchanged ---------------------------------------------------------------------------------------------
def test_classifier_step_is_bit_identical_before_and_after_an_encoder_backward():
    model = EG.build_model("rgb_56x70").train()
    src, tgt = synth.synth_volume((1, 1, 3, 56, 70), 7).cuda(), torch.tensor([1]).cuda()

    def step():
        for p in model.parameters():
            p.grad = None
        F.cross_entropy(model(src), tgt).backward()
        return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    with EG.deterministic():
        g1 = step()
        EG.device_grads(model, "rgb_56x70")
        g2 = step()
    assert set(g1) == set(g2) and len(g1) > 100
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
