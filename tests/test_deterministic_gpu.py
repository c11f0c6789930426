"""torch.use_deterministic_algorithms(True) on the HIP training steps and znormalize: the fixed-order entry points (csrc/k_colsum.hip, csrc/k_ordered.hip and
the ordered forms beside the atomic kernels) are bit-reproducible on inputs where the summation order visibly matters, agree with an fp64
reference and with the atomic kernels within fp32 reassociation error, are the ONLY reductions a step reaches under the flag, and make whole
training steps -- logits, loss, every gradient, BatchNorm running statistics -- bit-identical from run to run."""
import copy

import pytest
import torch

from mst import hip, synth

pytestmark = pytest.mark.gpu

ATOMIC = ("mst_colsum", "mst_layernorm_bwd", "mst_batchnorm_train", "mst_batchnorm_bwd", "mst_col2im_nhwc", "mst_maxpool_bwd_nhwc",
          "mst_pos_embed_interp_bwd", "mst_znorm")


@pytest.fixture
def det():
    prev, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev, warn_only=warn)


def _flag(on: bool):
    torch.use_deterministic_algorithms(on)


def _five(fn):
    """Five runs: each must be bit-identical to the first.  Returns the first."""
    first = fn()
    for _ in range(4):
        again = fn()
        for a, b in zip(first if isinstance(first, tuple) else (first,), again if isinstance(again, tuple) else (again,)):
            assert torch.equal(a, b)
    return first


def _cancelling(rows, cols, seed, big=1e7):
    """O(1) noise plus +-big entries that cancel inside every column: the fp32 sum depends on the order."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(rows, cols, device="cuda", generator=g)
    k = max(rows // 64, 2) // 2 * 2
    idx = torch.randperm(rows, device="cuda", generator=g)[:k]
    sign = torch.ones(k, 1, device="cuda")
    sign[k // 2:] = -1.0
    a[idx] += sign * big
    return a


def _colsum_case(a, b=None, out0=None, compare_atomic=True):
    rows, cols = a.shape
    base = out0 if out0 is not None else torch.zeros(cols, device="cuda")
    got = _five(lambda: hip.colsum(a, base.clone(), b=b))
    prod = a.double() if b is None else a.double() * b.double()
    ref = base.double() + prod.sum(0)
    scale = base.double().abs() + prod.abs().sum(0)
    assert float(((got.double() - ref).abs() - 2e-5 * scale).max()) <= 0.0
    if compare_atomic:
        _flag(False)
        try:
            atomic = hip.colsum(a, base.clone(), b=b)
        finally:
            _flag(True)
        assert float(((got.double() - atomic.double()).abs() - 4e-5 * scale).max()) <= 0.0
    return got


def test_ordered_colsum_at_the_stem_batchnorm_shape(det):
    a = _cancelling(2 * 128 * 256 * 256, 64, 1)                           # 16.8 M rows x 64 channels (2 x 128 x 512^2 step)
    _colsum_case(a)


def test_ordered_colsum_past_the_column_block_limit(det):
    a = _cancelling(16, 4194304, 2)                                       # ViT-L fc weight-gradient partials: 65,536 column blocks
    _colsum_case(a)                                                       # (one more than a gridDim.y: mst_colsum goes in two pieces)


def test_ordered_colsum_into_a_nonzero_out_with_b_and_a_strided_view(det):
    a = _cancelling(5000, 384, 3)
    b = torch.randn(5000, 384, device="cuda")
    out0 = torch.randn(384, device="cuda") * 100
    _colsum_case(a, b=b, out0=out0)
    wide = _cancelling(777, 3 * 388, 4)                                   # a column block of a wider matrix (the CLS / register rows)
    _colsum_case(wide[:, 388:2 * 388], out0=torch.randn(388, device="cuda"))
    _colsum_case(_cancelling(301, 37, 5))                                 # odd columns: the scalar loads


@pytest.mark.parametrize("bdt", [None, torch.float32, torch.bfloat16, torch.float16], ids=["no_b", "b_fp32", "b_bf16", "b_fp16"])
def test_colsum_single_row_block_atomic_equals_ordered_bits(det, bdt):
    """One row block (rows <= 64, the plan's minimum): the atomic and the ordered entry points are instantiations of one kernel
    (csrc/k_colsum.hip), walk the rows in the same order and add one total per column to `out` -- so the bits are equal.  cols: 4 and 64
    one column block, 68 a ragged second one, 388 the register-token width; contiguous 16-byte-aligned operands (the vector layout)."""
    g = torch.Generator(device="cuda").manual_seed(21)
    for rows in (1, 17, 64):
        for cols in (4, 64, 68, 388):
            a = torch.randn(rows, cols, device="cuda", generator=g) * 1e3
            b = None if bdt is None else torch.randn(rows, cols, device="cuda", generator=g).to(bdt)
            out0 = torch.randn(cols, device="cuda", generator=g) * 100
            ordered = hip.colsum(a, out0.clone(), b=b)
            _flag(False)
            try:
                atomic = hip.colsum(a, out0.clone(), b=b)
            finally:
                _flag(True)
            assert torch.equal(atomic, ordered), (rows, cols)
            prod = a.double() if b is None else a.double() * b.double()
            assert float(((ordered.double() - out0.double() - prod.sum(0)).abs() - 2e-5 * (out0.double().abs() + prod.abs().sum(0))).max()) <= 0.0


def test_batchnorm_single_row_block_atomic_equals_ordered_bits(det):
    """fp32 BatchNorm forward and backward with residual and ReLU, flag off against flag on, at one row block (rows <= 64, the plan's
    minimum).  Every sum of both modes -- sum z, sum (z - mean)^2, d gamma, d beta -- is an instantiation of ONE kernel
    (colreduce_kernel, csrc/k_colsum.hip) that walks the rows in the same order and adds one total per column to a zeroed output, and y
    and dz come from the same apply kernels (csrc/k_bn.hip): so every output has the same bits.  C: 4 and 64 one column block, 68 a ragged
    second one, 512 eight; contiguous 16-byte-aligned operands.
    Expected to FAIL on the library before the BatchNorm kernels were unified: its atomic sum (z - mean)^2, d gamma and d beta were
    kernels of their own (one thread per column down 256 rows), whose row order is not the ordered form's."""
    from mst.models.resnet import _BN
    g = torch.Generator(device="cuda").manual_seed(23)
    for rows in (1, 17, 64):
        for C in (4, 64, 68, 512):
            z = torch.randn(rows, C, device="cuda", generator=g) * 3 + 1
            res = torch.randn(rows, C, device="cuda", generator=g)
            dy = torch.randn(rows, C, device="cuda", generator=g)
            bn0 = _BN(C).cuda()
            with torch.no_grad():
                bn0.weight.copy_(torch.rand(C, device="cuda", generator=g) + 0.5)
                bn0.bias.copy_(torch.randn(C, device="cuda", generator=g) * 0.3)

            def run():
                bn = copy.deepcopy(bn0)
                y, mean, rstd = hip.batchnorm_train(z, bn, res, True)
                d = hip.act_bwd(y, dy.clone(), 1)
                dz, dg, db = hip.batchnorm_bwd(z, mean, rstd, bn.weight.detach(), d)
                return y, mean, rstd, bn.running_mean, bn.running_var, dz, dg, db

            ordered = run()
            _flag(False)
            try:
                atomic = run()
            finally:
                _flag(True)
            for name, a, o in zip(("y", "mean", "rstd", "running_mean", "running_var", "dz", "dgamma", "dbeta"), atomic, ordered):
                assert torch.equal(a, o), (rows, C, name)
            assert float(ordered[0].abs().sum()) > 0 and (rows == 1 or float(ordered[5].abs().sum()) > 0)    # one row: dz = 0


def test_gather_maxpool_backward_equals_the_atomic_kernel_on_ties(det):
    g = torch.Generator(device="cuda").manual_seed(6)
    for n, H, W, C in ((2, 65, 64, 64), (1, 32, 33, 16)):
        x = torch.relu(torch.randint(-3, 3, (n, H, W, C), device="cuda", generator=g).float())      # post-ReLU: mostly zeros and ties
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        dy = torch.randint(-8, 9, (n, Ho, Wo, C), device="cuda", generator=g).float()              # small integers: every sum is exact
        got = _five(lambda: hip.maxpool_bwd_nhwc(x, dy))
        _flag(False)
        try:
            atomic = hip.maxpool_bwd_nhwc(x, dy)
        finally:
            _flag(True)
        assert torch.equal(got, atomic)


def test_gather_col2im_equals_the_adjoint_of_im2col(det):
    g = torch.Generator(device="cuda").manual_seed(7)
    for n, H, W, C, k, s, p in ((2, 17, 18, 8, 3, 2, 1), (1, 20, 20, 4, 7, 2, 3), (2, 9, 9, 16, 1, 1, 0)):
        x = torch.randn(n, H, W, C, device="cuda", generator=g)
        col = hip.im2col_nhwc(x, k, k, s, p)
        dcol = torch.randn(col.shape, device="cuda", generator=g) * 1e3
        dx0 = torch.randn(n, H, W, C, device="cuda", generator=g)
        got = _five(lambda: hip.col2im_nhwc(dcol, dx0.clone(), k, k, s, p))
        # <col2im(dcol), x> == <dcol, im2col(x)> in fp64, and the atomic kernel within reassociation error
        lhs = float(((got - dx0).double() * x.double()).sum())
        K = k * k * C
        rhs = float((dcol[:, :K].double() * col[:, :K].double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float((dcol[:, :K].double().abs() * col[:, :K].double().abs()).sum())
        _flag(False)
        try:
            atomic = hip.col2im_nhwc(dcol, dx0.clone(), k, k, s, p)
        finally:
            _flag(True)
        assert float((got - atomic).abs().max()) <= 1e-5 * float(dcol.abs().max()) * k * k


def test_ordered_pos_embed_adjoint_against_a_dense_fp64_adjoint(det):
    M, gh, gw, E = 37, 16, 16, 384
    # the dense interpolation matrix A [gh*gw, M*M] from the forward kernel applied to the identity (the clamped edge taps included)
    A = hip.pos_embed_interp(torch.eye(M * M, device="cuda"), M, gh, gw, 0.1).double()
    g = torch.Generator(device="cuda").manual_seed(8)
    dout = torch.randn(gh * gw, E, device="cuda", generator=g)
    dout[::7] *= 1e6
    dpos0 = torch.randn(M * M, E, device="cuda", generator=g)
    got = _five(lambda: hip.pos_embed_interp_bwd(dout, M, gh, gw, 0.1, dpos0.clone()))
    ref = dpos0.double() + A.t() @ dout.double()
    scale = dpos0.double().abs() + A.abs().t() @ dout.double().abs()
    assert float(((got.double() - ref).abs() - 1e-5 * scale).max()) <= 0.0
    edge = torch.zeros(M, M, dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    assert float((got - dpos0)[edge.view(-1).cuda()].abs().max()) > 0        # the clamped border cells receive gradient
    _flag(False)
    try:
        atomic = hip.pos_embed_interp_bwd(dout, M, gh, gw, 0.1, dpos0.clone())
    finally:
        _flag(True)
    assert float(((got.double() - atomic.double()).abs() - 2e-5 * scale).max()) <= 0.0


def test_ordered_layernorm_and_batchnorm_reductions(det):
    g = torch.Generator(device="cuda").manual_seed(9)
    rows, cols = 4112, 384
    x = torch.randn(rows, cols, device="cuda", generator=g) * 3 + 1
    dy = _cancelling(rows, cols, 10, big=1e4)
    gamma = torch.randn(cols, device="cuda", generator=g)

    def ln():
        dx = torch.empty(rows, cols, device="cuda")
        dg, db = torch.zeros(cols, device="cuda"), torch.zeros(cols, device="cuda")
        hip.layernorm_bwd(x, cols, gamma, dy, cols, None, 0, dx, cols, dg, db, rows, cols, 1e-6)
        return dx, dg, db
    dx, dg, db = _five(ln)
    _flag(False)
    try:
        dxa, dga, dba = ln()
    finally:
        _flag(True)
    assert torch.equal(dx, dxa)                                           # dx is computed exactly as before
    xh = (x.double() - x.double().mean(1, keepdim=True)) / (x.double().var(1, unbiased=False, keepdim=True) + 1e-6).sqrt()
    for got, atomic, ref, sc in ((dg, dga, (dy.double() * xh).sum(0), (dy.double() * xh).abs().sum(0)),
                                 (db, dba, dy.double().sum(0), dy.double().abs().sum(0))):
        assert float(((got.double() - ref).abs() - 2e-5 * sc).max()) <= 0.0
        assert float(((got.double() - atomic.double()).abs() - 4e-5 * sc).max()) <= 0.0

    bn = torch.nn.BatchNorm2d(64).cuda()
    with torch.no_grad():
        bn.weight.normal_()
        bn.bias.normal_()
    z = torch.randn(300000, 64, device="cuda", generator=g) * 5 + 2
    dyz = torch.sin(z) * 1e3

    def bnrun():
        b = copy.deepcopy(bn)
        y, mean, rstd = hip.batchnorm_train(z, b, None, True)
        dz, dgb, dbb = hip.batchnorm_bwd(z, mean, rstd, b.weight.detach(), dyz)
        return y, mean, rstd, b.running_mean, b.running_var, dz, dgb, dbb
    det_out = _five(bnrun)
    _flag(False)
    try:
        at_out = bnrun()
    finally:
        _flag(True)
    for a, b in zip(det_out, at_out):
        assert float((a - b).abs().max()) <= 1e-4 * max(float(b.abs().max()), 1.0)
    mean_ref = z.double().mean(0)
    assert float((det_out[1].double() - mean_ref).abs().max()) < 1e-5


def test_znormalize_with_percentiles_is_bit_reproducible(det):
    from mst.preprocess import znormalize
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(1, 40, 96, 96, device="cuda", generator=g) * 300 + 1000
    x[0, :, :5] = 1e7                                                     # a large clamped tail
    out, st = znormalize(x, (0.5, 99.5), return_stats=True)
    for _ in range(4):
        o2, s2 = znormalize(x, (0.5, 99.5), return_stats=True)
        assert torch.equal(out, o2) and s2 == st
    _flag(False)
    try:
        oa, sa = znormalize(x, (0.5, 99.5), return_stats=True)
    finally:
        _flag(True)
    assert st["count"] == sa["count"] and st["cut_lo"] == sa["cut_lo"] and st["cut_hi"] == sa["cut_hi"]
    assert abs(st["mean"] - sa["mean"]) <= 1e-6 * abs(sa["mean"]) and abs(st["std"] - sa["std"]) <= 1e-6 * sa["std"]
    assert float((out - oa).abs().max()) < 1e-4


# ---- whole steps -------------------------------------------------------------------------------------------------------------------
def _dino(prec="fp32", attn="stored", **kw):
    from mst.models import DinoV2ClassifierSlice
    m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, train_precision=prec, train_attention=attn, **kw)
    m.load_state_dict(synth.synth_state_dict("s", 0, rotary=kw.get("rotary_positional_encoding")))
    return m.cuda().train()


def _resnet(prec="fp32"):
    from mst.models import ResNetSliceTrans
    m = ResNetSliceTrans(in_ch=1, out_ch=2, pretrained=False, model=34, train_precision=prec)
    m.load_state_dict(synth.synth_resnet_state_dict(0, 34, 2), strict=True)
    return m.cuda().train()


def _registers():
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    sd = synth.synth_state_dict("s", 23, img_size=56, layerscale=True, chunked=False, num_register_tokens=4)
    m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_registers=True)
    m.encoder = _ViT(384, 12, 6, img_size=56, num_register_tokens=4, layerscale=1.0, chunked=False)
    m.load_state_dict(sd, strict=True)
    return m.cuda().train()


def _step(model, src, mask=None):
    model.zero_grad(set_to_none=True)
    logits = model(src) if mask is None else model(src, src_key_padding_mask=mask)
    loss = torch.nn.functional.cross_entropy(logits, torch.arange(src.shape[0], device="cuda") % 2)
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    bufs = {k: b.detach().clone() for k, b in model.named_buffers() if b.is_floating_point()}
    return logits.detach().clone(), loss.detach().clone(), grads, bufs


def test_no_atomic_reduction_is_reached_under_the_flag(det, monkeypatch):
    lib = hip.load()

    def stub(name):
        def f(*args):
            raise AssertionError(f"{name}: an atomic reduction was reached with torch.use_deterministic_algorithms(True)")
        return f
    for name in ATOMIC:
        monkeypatch.setattr(lib, name, stub(name))
    src = synth.synth_volume((2, 1, 4, 224, 224), 3).cuda()
    for prec, attn in (("fp32", "stored"), ("fp16", "flash"), ("bf16", "stored"), ("bf16", "flash"), ("fp16", "stored")):
        _step(_dino(prec, attn), src)
    _step(_dino(rotary_positional_encoding="RoPE"), src)
    mask = torch.zeros(2, 4, dtype=torch.bool)
    mask[1, 2:] = True
    _step(_dino(), src, mask.cuda())
    _step(_registers(), synth.synth_volume((2, 1, 3, 56, 56), 123).cuda())
    rsrc = synth.synth_volume((2, 1, 3, 96, 96), 4).cuda()
    for prec in ("fp32", "fp16", "bf16"):
        _step(_resnet(prec), rsrc)
    monkeypatch.setenv("MST_CONV_IM2COL", "1")                            # the explicit forms: col2im of every input gradient
    _step(_resnet("fp32"), rsrc)
    from mst.preprocess import znormalize
    znormalize(synth.synth_volume((1, 1, 8, 64, 64), 5)[0].cuda(), (0.5, 99.5))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("family,prec,attn,bar", [("dino", "fp32", "stored", 1e-5), ("dino", "fp16", "flash", 1e-2),
                                                   ("dino", "bf16", "stored", 1.3e-1), ("resnet", "fp32", None, 0.1),
                                                   ("resnet", "fp16", None, 0.5)])
def test_training_steps_are_bit_reproducible(det, family, prec, attn, bar):
    """Two steps from the same state: bit-identical.  Against the flag-off (atomic) step: DINOv2 within the bars of the fp32 and mixed
    precision tests (relative L2 per parameter); the ResNet step is ill-conditioned -- the flag-off step is not even run-to-run identical,
    ReLU flips behind train-mode BatchNorm move whole upstream gradients (test_resnet_gpu.py::test_training_step_matches_autograd_of_oracle)
    -- so its fp32 bar is that test's: every parameter within 10 %, the median within 5 %; in fp16 a rounding of the 16-bit operands moves
    these gradients by 0.2 .. 0.5, which is its bar (measured against the flag-off step: 0.21 worst, 0.16 median)."""
    if family == "dino":
        model, src = _dino(prec, attn), synth.synth_volume((2, 1, 16, 224, 224), 3).cuda()
    else:
        model, src = _resnet(prec), synth.synth_volume((2, 1, 8, 128, 128), 4).cuda()
    state = copy.deepcopy(model.state_dict())

    def run():
        model.load_state_dict(state)
        return _step(model, src)
    l1, loss1, g1, b1 = run()
    l2, loss2, g2, b2 = run()
    assert torch.equal(l1, l2) and torch.equal(loss1, loss2)
    assert set(g1) == set(g2) and len(g1) > 0
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
        assert bool(torch.isfinite(g1[k]).all()), k                      # no uninitialised (NaN-filled) memory read
    for k in b1:
        assert torch.equal(b1[k], b2[k]), k                              # BatchNorm running statistics
    _flag(False)
    try:
        l0, loss0, g0, _ = run()
    finally:
        _flag(True)
    assert float((l1 - l0).abs().max()) <= max(bar, 1e-4)
    errs = [_rel(g1[k], g0[k]) for k in g0 if float(g0[k].abs().max()) > 0]
    print(family, prec, attn, "gradients against the flag-off step: worst", max(errs), "median", sorted(errs)[len(errs) // 2])
    assert max(errs) <= bar, max(errs)
    if family == "resnet":
        assert sorted(errs)[len(errs) // 2] <= bar / 2
