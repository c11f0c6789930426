"""train_storage='16bit' of the ResNet / ResNetSliceTrans training step (csrc/k_bn.hip, mst/train_resnet.py) and the autocast rule of
their train_precision: the new entry points against fp64 on the same 16-bit inputs and against the fp32 entry points on the upcast inputs,
one convolution + BatchNorm unit forward and backward against fp64 torch with the same roundings inserted, whole models (finite gradients,
loss, the bytes the saved state takes, peak memory), determinism, autocast.

Where the bounds come from.  T has 11 (fp16) / 8 (bf16) significant bits, fp32 24.
  * A kernel value is T(an fp32 evaluation of the formula).  Against the fp64 value v it is off by at most half an ulp of T from the
    rounding, plus what the fp32 evaluation is off by, which can also move the rounding by one step: 1 ulp of T at v, plus a few fp32
    epsilons (6e-8) times the magnitude of every term that enters -- with z - mean expanded, because the fp32 mean carries its own relative
    error: 4e-7 * sum |terms| allows six of them.
  * The share of elements where the kernel differs from T(v) at all is the chance that v lies within the fp32 error of a rounding boundary of
    T: (fp32 error) / (half an ulp of T), of the order of 1e-3 for fp16 and less for bf16; the bar is 0.5 %.
  * Sums over rows (mean, variance, d gamma, d beta) are fp32 sums of exactly known inputs in a blocked order: 1e-5 / 2e-5 relative.
  * One unit against fp64: the convolution accumulates in fp32 in the MFMA's order, so a few elements per thousand of z land on the other side
    of a rounding boundary of T (one ulp of T each): 2e-4 rel-L2.
Figures measured on an MI355X are in the docstrings of the tests."""

import contextlib
import copy
import warnings

import pytest
import torch

from conftest import rel_l2
from mst import synth

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
EINVAL = 1


@contextlib.contextmanager
def _deterministic():
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(was)


def _ulp(v: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """Spacing of T at the fp64 value v (the subnormal spacing below the smallest normal)."""
    mant, emin = (10, -14) if dt == torch.float16 else (7, -126)
    e = torch.frexp(v.abs().clamp_min(2.0 ** emin))[1] - 1               # floor(log2 |v|)
    return torch.pow(torch.full_like(v, 2.0), (e - mant).to(v.dtype))


def _bn(C, g, dev="cuda"):
    from mst.models.resnet import _BN
    bn = _BN(C)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return bn.to(dev)


def _stats64(z16: torch.Tensor, eps: float):
    zf = z16.double()
    mu = zf.mean(0)
    var = ((zf - mu) ** 2).mean(0)
    return zf, mu, var, (var + eps) ** -0.5


# ---- 1. the BatchNorm kernels against fp64 on the same 16-bit inputs -------------------------------------------------------------------

BN_SHAPES = [(385, 64), (140, 128), (2051, 256), (33, 2048), (70001, 64)]


@pytest.mark.parametrize("residual,relu", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("rows,C", BN_SHAPES)
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_batchnorm16_forward_and_backward_against_fp64(prec, rows, C, residual, relu):
    """One column group (C = 64), odd row counts, the widest layer (C = 2048) and more row blocks than one workgroup sees (70001 rows: 1,094
    blocks of 64 rows).  z is normal with a per-channel scale in [0.5, 2] and offset in [-1, 1]; residual and dy of unit scale.

    The terms of dz: m dy, and the SUMMANDS of d beta / rows and of xhat d gamma / rows (xhat with z - mean expanded).  A first version of
    this test took |d beta| / rows and |d gamma| / rows themselves; at bf16 2051 x 256 with ReLU two ReLU-masked elements, where dz is
    the nearly cancelling difference of those two terms (|dz| = 2e-9 against terms of 1e-3), missed that bound by 1.3e-9 and 7.5e-10.
    An fp32 sum of 2,051 signed values is not accurate to a few epsilons of its own (cancelled) total -- torch's fp32 sums on the CPU
    miss that version at the same elements (2.6e-10) -- so that reading asked what no fp32 reduction gives; its error is a few epsilons
    of the summands' magnitudes, which is what the bound now counts.  Everywhere else the ulp term decides.
    Measured (MI355X): y differs from T(fp64) on at most 0.065 % of the elements (fp16) / 0.020 % (bf16), dz on 0.100 % / 0.022 %."""
    from mst import hip
    dt = DT[prec]
    g = torch.Generator().manual_seed(1000 + rows + C)
    scale, offset = torch.rand(C, generator=g) * 1.5 + 0.5, torch.rand(C, generator=g) * 2 - 1
    z = (torch.randn(rows, C, generator=g) * scale + offset).to(dt).cuda()
    res = torch.randn(rows, C, generator=g).to(dt).cuda() if residual else None
    dy0 = torch.randn(rows, C, generator=g).cuda()
    bn = _bn(C, g)
    bn2 = copy.deepcopy(bn)
    rm0, rv0 = bn.running_mean.double().clone(), bn.running_var.double().clone()
    gam, bet = bn.weight.detach().double(), bn.bias.detach().double()

    y, mean, rstd = hip.batchnorm_train16(z, bn, res, relu)
    zf, mu, var, rs = _stats64(z, bn.eps)
    assert rel_l2(mean, mu) < 1e-5 and rel_l2(rstd, rs) < 1e-5
    assert rel_l2(bn.running_mean, 0.9 * rm0 + 0.1 * mu) < 1e-5
    assert rel_l2(bn.running_var, 0.9 * rv0 + 0.1 * var * rows / (rows - 1)) < 1e-5
    v = gam * (zf - mu) * rs + bet
    terms = (gam * rs).abs() * (zf.abs() + mu.abs()) + bet.abs()
    if residual:
        v, terms = v + res.double(), terms + res.double().abs()
    if relu:
        v = v.clamp_min(0)
    assert y.dtype == dt and y.shape == z.shape
    err = (y.double() - v).abs()
    assert bool((err <= _ulp(v, dt) + 4e-7 * terms).all()), float((err - _ulp(v, dt) - 4e-7 * terms).max())
    share = float((y != v.to(dt)).double().mean())
    print(f"batchnorm_train16 {prec} {rows}x{C} res={residual} relu={relu}: y differs from T(fp64) on {share:.3%}")
    assert share <= 0.005

    # the same call again (a copy of the module as it was): the same bits, determinism flag off
    y2, mean2, rstd2 = hip.batchnorm_train16(z, bn2, res, relu)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    assert torch.equal(bn.running_mean, bn2.running_mean) and torch.equal(bn.running_var, bn2.running_var)

    # backward on the kernel's own y (the ReLU mask) and statistics
    yk = y if relu else None
    m = (y > 0).double() if relu else torch.ones_like(zf)
    dy = dy0.clone()
    dz, dg, db = hip.batchnorm_bwd16(z, yk, mean, rstd, bn.weight.detach(), dy, False)
    assert torch.equal(dy, dy0)                                          # not asked to write the masked gradient back
    dyf = dy0.double() * m
    xh = (zf - mu) * rs
    db64, dg64 = dyf.sum(0), (dyf * xh).sum(0)
    assert rel_l2(db, db64) < 2e-5 and rel_l2(dg, dg64) < 2e-5
    v = gam * rs * (dyf - db64 / rows - xh * dg64 / rows)
    # d beta and d gamma are fp32 SUMS: what they are off by scales with the magnitude of their summands, not of the (possibly cancelled) total
    terms = (gam * rs).abs() * (dyf.abs() + dyf.abs().sum(0) / rows + rs * (zf.abs() + mu.abs()) * (dyf * xh).abs().sum(0) / rows)
    assert dz.dtype == dt
    err = (dz.double() - v).abs()
    assert bool((err <= _ulp(v, dt) + 4e-7 * terms).all()), float((err - _ulp(v, dt) - 4e-7 * terms).max())
    share = float((dz != v.to(dt)).double().mean())
    print(f"batchnorm_bwd16   {prec} {rows}x{C} res={residual} relu={relu}: dz differs from T(fp64) on {share:.3%}")
    assert share <= 0.005
    # with the masked gradient written back: dy * (y > 0) bit for bit, and every output the bits of the first call
    dzb, dgb, dbb = hip.batchnorm_bwd16(z, yk, mean, rstd, bn.weight.detach(), dy, True)
    assert torch.equal(dy, dy0 * (y > 0) if relu else dy0)
    assert torch.equal(dz, dzb) and torch.equal(dg, dgb) and torch.equal(db, dbb)


def test_batchnorm16_rejects_what_it_cannot_take():
    from mst import hip
    lib = hip.load()
    rows, C = 96, 64
    z = torch.zeros(rows + 1, C, dtype=torch.float16, device="cuda")
    y = torch.empty_like(z)
    dy = torch.zeros(rows + 1, C, device="cuda")
    vec = [torch.ones(C, device="cuda") for _ in range(6)]
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    s = hip.stream_of(z)
    f16 = hip.dt_of(z)

    def fwd(zp, c, wsb, dtype=f16):
        return lib.mst_batchnorm_train16(zp, dtype, rows, c, hip.ptr(vec[0]), hip.ptr(vec[1]), 1e-5, 0.1, None, 1, hip.ptr(y), hip.ptr(vec[2]),
                                         hip.ptr(vec[3]), None, None, hip.ptr(ws), wsb, s)

    def bwd(zp, c, wsb, dtype=f16):
        return lib.mst_batchnorm_bwd16(zp, None, dtype, hip.ptr(vec[2]), hip.ptr(vec[3]), hip.ptr(vec[0]), hip.ptr(dy), 0, rows, c, hip.ptr(vec[4]),
                                       hip.ptr(vec[5]), hip.ptr(y), hip.ptr(ws), wsb, s)

    need_f, need_b = lib.mst_batchnorm_train16_workspace_bytes(rows, C), lib.mst_batchnorm_bwd16_workspace_bytes(rows, C)
    assert 0 < need_f <= ws.numel() and 0 < need_b <= ws.numel()
    for call, need in ((fwd, need_f), (bwd, need_b)):
        assert call(hip.ptr(z), C, ws.numel()) == 0
        assert call(hip.ptr(z), 60, ws.numel()) == EINVAL                 # C not a multiple of 8
        assert call(hip.ptr(z) + 2, C, ws.numel()) == EINVAL              # a base off the 16-byte grid
        assert call(hip.ptr(z), C, need - 1) == EINVAL                    # a short workspace
        assert call(hip.ptr(z), C, ws.numel(), 0) == EINVAL               # fp32 is not a 16-bit type
        assert "batchnorm" in hip.last_error()
    assert lib.mst_batchnorm_train16_workspace_bytes(rows, 60) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("residual,relu", [(False, False), (False, True), (True, True)])
@pytest.mark.parametrize("C", [8, 64, 136])
@pytest.mark.parametrize("rows", [1, 9, 16])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_batchnorm16_is_the_fp32_entry_point_on_the_upcast_input(prec, rows, C, residual, relu):
    """Under the determinism flag the 16-bit and the fp32 BatchNorm are one kernel family (csrc/k_bn.hip, colreduce_kernel of
    csrc/k_colsum.hip): the same expressions on the same fp32 values.  The two column-sum geometries differ in their thread rows (32 for
    a 16-bit z, 16 for fp32), but up to 16 rows every thread row of either holds at most one row, so the LDS sums add the same values in
    the same ascending order (the rest are zeros) and the statistics agree BITWISE; y and dz are then T(the fp32 result).  C: 8 one lane,
    64 one column block, 136 a ragged third one."""
    from mst import hip
    dt = DT[prec]
    g = torch.Generator().manual_seed(2000 + rows + C)
    z16 = (torch.randn(rows, C, generator=g) * 2 + 0.5).to(dt).cuda()
    res16 = torch.randn(rows, C, generator=g).to(dt).cuda() if residual else None
    dy = torch.randn(rows, C, generator=g).cuda()
    bn16 = _bn(C, g)
    bn32 = copy.deepcopy(bn16)
    gamma = bn16.weight.detach()
    with _deterministic():
        y32, mean32, rstd32 = hip.batchnorm_train(z16.float(), bn32, None if res16 is None else res16.float(), relu)
        y16, mean16, rstd16 = hip.batchnorm_train(z16, bn16, res16, relu)
        assert y16.dtype == dt and y32.dtype == torch.float32
        assert torch.equal(mean16, mean32) and torch.equal(rstd16, rstd32)
        assert torch.equal(bn16.running_mean, bn32.running_mean) and torch.equal(bn16.running_var, bn32.running_var)
        assert torch.equal(y16, y32.to(dt))
        dy32 = hip.act_bwd(y16.float(), dy.clone(), 1) if relu else dy.clone()
        dz32, dg32, db32 = hip.batchnorm_bwd(z16.float(), mean32, rstd32, gamma, dy32)
        dz16, dg16, db16 = hip.batchnorm_bwd16(z16, y16 if relu else None, mean16, rstd16, gamma, dy.clone(), False)
    assert dz16.dtype == dt and torch.equal(dz16, dz32.to(dt))
    assert torch.equal(dg16, dg32) and torch.equal(db16, db32)


# ---- 2. the pools ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(3, 9, 7, 64), (2, 16, 16, 128)])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_maxpool_backward_on_16_bit_input_is_the_gather_form_on_the_upcast_input(prec, shape):
    from mst import hip
    g = torch.Generator().manual_seed(31)
    n, H, W, C = shape
    x = torch.randn(shape, generator=g).clamp_min(0).to(DT[prec]).cuda()           # post-ReLU: every window of zeros is a tie
    dy = torch.randn(n, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C, generator=g).cuda()
    got = hip.maxpool_bwd_nhwc(x, dy)
    with _deterministic():
        ref = hip.maxpool_bwd_nhwc(x.float(), dy)                                  # mst_maxpool_bwd_nhwc_gather
    assert got.dtype == torch.float32 and torch.equal(got, ref)
    assert float(got.abs().sum()) > 0
    lib = hip.load()
    need = lib.mst_maxpool_bwd_nhwc16_workspace_bytes(n, H, W, C)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    bad = (lib.mst_maxpool_bwd_nhwc16(hip.ptr(x), hip.dt_of(x), hip.ptr(dy), n, H, W, C, hip.ptr(got), hip.ptr(ws), need - 1, hip.stream_of(x)),
           lib.mst_maxpool_bwd_nhwc16(hip.ptr(x), hip.dt_of(x), hip.ptr(dy), n, H, W, 60, hip.ptr(got), hip.ptr(ws), need, hip.stream_of(x)),
           lib.mst_maxpool_bwd_nhwc16(hip.ptr(x) + 2, hip.dt_of(x), hip.ptr(dy), n, H, W, C, hip.ptr(got), hip.ptr(ws), need, hip.stream_of(x)))
    assert bad == (EINVAL, EINVAL, EINVAL)


@pytest.mark.parametrize("shape", [(3, 9, 7, 64), (2, 16, 16, 128), (5, 3, 3, 2048)])
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_avgpool_on_16_bit_input_is_the_fp32_pool_on_the_upcast_input(prec, shape):
    from mst import hip
    x = torch.randn(shape, generator=torch.Generator().manual_seed(32)).to(DT[prec]).cuda()
    got = hip.avgpool_nhwc(x)
    assert got.dtype == torch.float32 and torch.equal(got, hip.avgpool_nhwc(x.float()))
    lib = hip.load()
    n, H, W, C = shape
    assert lib.mst_avgpool_nhwc16(hip.ptr(x), hip.dt_of(x), n, H * W, 60, hip.ptr(got), hip.stream_of(x)) == EINVAL
    assert lib.mst_avgpool_nhwc16(hip.ptr(x) + 2, hip.dt_of(x), n, H * W, C, hip.ptr(got), hip.stream_of(x)) == EINVAL


# ---- 3. / 4. one unit, forward and backward ---------------------------------------------------------------------------------------------

#             cin cout k  s  p  (H, W)   residual relu  stem
UNIT_CASES = {
    "3x3_s2": (64, 128, 3, 2, 1, (22, 18), False, True, False),
    "3x3_residual_128": (128, 128, 3, 1, 1, (12, 10), True, True, False),
    "1x1_s2_no_relu": (64, 256, 1, 2, 0, (12, 10), False, False, False),
    "3x3_residual_64": (64, 64, 3, 1, 1, (14, 12), True, True, False),
    "stem_7x7": (1, 64, 7, 2, 3, (40, 36), False, True, True),
}


@pytest.mark.parametrize("case", list(UNIT_CASES))
@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_one_unit_forward_and_backward_against_fp64_with_the_same_roundings(prec, case):
    """Forward: torch in fp64 with weight and input rounded to T, z rounded to T, BatchNorm in fp64, + float(residual), ReLU, rounded to T.
    Backward: the fp64 reference is taken from the HIP record (mask = y16 > 0, xhat from the upcast z16 with fp64 statistics), dz rounded to
    T, torch.nn.grad.conv2d_weight / conv2d_input in fp64 on the T-rounded operands.
    Measured (MI355X), bar 2e-4: y at most 2.1e-5 (fp16) / 9.5e-5 (bf16, the stem); dW, dx at most 6.8e-6 / 4.8e-5; d gamma, d beta 1.5e-7;
    running statistics at most 8.2e-7 (bar 1e-5)."""
    import torch.nn.functional as F
    from mst import train_resnet as T
    from mst.models.resnet import _Conv
    dt = DT[prec]
    cin, cout, k, stride, pad, hw, residual, relu, stem = UNIT_CASES[case]
    n = 4
    g = torch.Generator().manual_seed(77)
    torch.manual_seed(77)                                # _Conv draws its kaiming weights from the global generator
    conv, bn = _Conv(3 if stem else cin, cout, k).cuda(), _bn(cout, g)
    rm0, rv0 = bn.running_mean.double().cpu().clone(), bn.running_var.double().cpu().clone()
    x = torch.randn(n, hw[0], hw[1], cin, generator=g)
    x = x.cuda() if stem else x.to(dt).cuda()            # a unit behind the stem takes its input already in T
    Ho, Wo = (hw[0] + 2 * pad - k) // stride + 1, (hw[1] + 2 * pad - k) // stride + 1
    rows = n * Ho * Wo
    res = torch.randn(rows, cout, generator=g).to(dt).cuda() if residual else None
    dy0 = torch.randn(rows, cout, generator=g).cuda()

    y, rec = T._conv_bn_fwd(x, conv, bn, k, stride, pad, stem, res, relu, dt, True)

    # -- the record: nothing fp32 but the [C] vectors (and the stem's source images), no copy of the input
    assert y.dtype == dt and y.shape == (n, Ho, Wo, cout)
    assert rec["z"].dtype == dt and rec["mp"] == dt
    assert (rec["y"] is None) == (not relu) and (rec["y"] is None or rec["y"].dtype == dt)
    assert rec["x"].data_ptr() == x.data_ptr()
    assert rec.get("x16") is None or rec["x16"] is rec["x"]
    for key, t in rec.items():
        if torch.is_tensor(t) and t.dtype == torch.float32:
            assert t.shape == (cout,) or (stem and key == "x"), (key, tuple(t.shape))
    assert (rec["col16"] is not None) == stem and (not stem or rec["col16"].dtype == dt)

    # -- forward against fp64
    w_eff = conv.weight.detach().sum(dim=1, keepdim=True) if stem else conv.weight.detach()
    xT, wT = x.to(dt).double().cpu().permute(0, 3, 1, 2), w_eff.to(dt).double().cpu()
    z64 = F.conv2d(xT, wT, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(rows, cout)
    gam, bet = bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu()
    zf, mu, var, rs = _stats64(z64.to(dt), bn.eps)
    v = gam * (zf - mu) * rs + bet
    if residual:
        v = v + res.double().cpu()
    if relu:
        v = v.clamp_min(0)
    e_y = rel_l2(y.reshape(rows, cout).cpu(), v.to(dt))
    e_rm = rel_l2(bn.running_mean.cpu(), 0.9 * rm0 + 0.1 * mu)
    e_rv = rel_l2(bn.running_var.cpu(), 0.9 * rv0 + 0.1 * var * rows / (rows - 1))
    print(f"unit {case} {prec}: y {e_y:.2e} running mean {e_rm:.2e} var {e_rv:.2e}")
    assert e_y < 2e-4 and e_rm < 1e-5 and e_rv < 1e-5
    assert int(bn.num_batches_tracked) == 1

    # -- backward on the forward's own saved tensors
    G = T._Grads()
    dy = dy0.clone()
    dx = T._conv_bn_bwd(G, rec, dy, not stem, True)
    m = (rec["y"] > 0) if relu else torch.ones_like(rec["z"], dtype=torch.bool)
    assert torch.equal(dy, dy0 * m)                                      # the masked gradient, bit for bit
    zf, mu, var, rs = _stats64(rec["z"].cpu(), bn.eps)
    dyf = dy0.double().cpu() * m.double().cpu()
    xh = (zf - mu) * rs
    db64, dg64 = dyf.sum(0), (dyf * xh).sum(0)
    dz64 = (gam * rs * (dyf - db64 / rows - xh * dg64 / rows)).to(dt).double()
    dzn = dz64.reshape(n, Ho, Wo, cout).permute(0, 3, 1, 2)
    dw64 = torch.nn.grad.conv2d_weight(xT, wT.shape, dzn, stride=stride, padding=pad)
    if stem:
        dw64 = dw64.expand(cout, 3, k, k)
    errs = {"dW": rel_l2(G.by_param[id(conv.weight)].cpu(), dw64), "dgamma": rel_l2(G.by_param[id(bn.weight)].cpu(), dg64),
            "dbeta": rel_l2(G.by_param[id(bn.bias)].cpu(), db64)}
    if not stem:
        dx64 = torch.nn.grad.conv2d_input(xT.shape, conv.weight.detach().to(dt).double().cpu(), dzn, stride=stride, padding=pad)
        assert dx.dtype == torch.float32
        errs["dx"] = rel_l2(dx.cpu().permute(0, 3, 1, 2), dx64)
    print(f"unit {case} {prec}: " + " ".join(f"{k_} {e:.2e}" for k_, e in errs.items()))
    assert all(e < 2e-4 for e in errs.values()), errs


def test_a_unit_that_cannot_take_the_16_bit_products_raises():
    from mst import train_resnet as T
    from mst.models.resnet import _Conv
    g = torch.Generator().manual_seed(3)
    conv, bn = _Conv(32, 64, 3).cuda(), _bn(64, g)
    x = torch.randn(2, 8, 8, 32, generator=g).half().cuda()
    with pytest.raises(ValueError, match="16bit"):
        T._conv_bn_fwd(x, conv, bn, 3, 1, 1, False, None, True, torch.float16, True)


# ---- 5. whole models ---------------------------------------------------------------------------------------------------------------------

SHAPE = (2, 1, 4, 96, 64)


def _slice_model(prec=None, storage=None, model=34, seed=41):
    from mst.models import ResNetSliceTrans
    kw = {}
    if prec is not None:
        kw["train_precision"] = prec
    if storage is not None:
        kw["train_storage"] = storage
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ResNetSliceTrans(in_ch=1, out_ch=2, pretrained=False, model=model, **kw)
    m.load_state_dict(synth.synth_resnet_state_dict(seed, model, 2), strict=True)
    return m.cuda().train()


def _tensors(obj, out):
    if torch.is_tensor(obj):
        out.append(obj)
    elif isinstance(obj, dict):
        for key, v in obj.items():
            if key not in ("conv", "bn"):                # the modules own the parameters: not saved state
                _tensors(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _tensors(v, out)
    return out


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_whole_model_step_loss_and_adamw(prec):
    """Every gradient finite, the first loss within 10 % of the fp32 step's (the functional bar of the mixed-precision test for this
    ill-conditioned net), four AdamW steps lower it.  Measured: first loss 1.2068 (fp16) / 1.2530 (bf16) against 1.2045."""
    src = synth.synth_volume(SHAPE, 42).cuda()
    tgt = torch.tensor([1, 0]).cuda()
    ref = float(torch.nn.functional.cross_entropy(_slice_model("fp32")(src), tgt).detach())
    m = _slice_model(prec, "16bit")
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    hist = []
    for _ in range(4):
        opt.zero_grad()
        logits = m(src)
        assert logits.dtype == torch.float32
        loss = torch.nn.functional.cross_entropy(logits, tgt)
        loss.backward()
        assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in m.parameters())
        opt.step()
        hist.append(float(loss.detach()))
    print(f"16bit storage {prec}: losses {hist}, fp32 step {ref:.4f}")
    assert abs(hist[0] - ref) < 0.1 * ref, (hist, ref)
    assert hist[-1] < hist[0], hist


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_saved_state_is_as_small_as_the_model_says_and_peak_memory_drops(prec):
    """The unique storages of the saved backbone state take 2 bytes per element of every z and y, plus col16, plus the max-pool output (within
    1 %); nothing in it is fp32 but the [C] vectors and the source volume; a step's peak memory is below the fp32-storage step's.
    Measured: 16,269,312 bytes saved = the model exactly; peak 317,429,760 -> 209,950,720 bytes."""
    from mst import train_resnet as T
    dt = DT[prec]
    src = synth.synth_volume(SHAPE, 42).cuda()
    B, _, D, H, W = SHAPE
    x = src.float().reshape(B * D, H, W, 1).contiguous()
    m = _slice_model(prec, "16bit")
    with torch.no_grad():
        _, sv = T.forward_train(m, x, True, B, D, None)
    assert sv["storage"] == "16bit" and sv["mp"] == dt
    recs = [sv["stem"]] + [r for unit in sv["units"] for r in unit if r is not None]
    assert len(recs) == 1 + 16 * 2 + 3 and all(r["mp"] == dt and r["storage16"] for r in recs)
    state = {k: sv[k] for k in ("stem", "units", "pool_in", "last")}
    seen, total = set(), 0
    for t in _tensors(state, []):
        if t.dtype == torch.float32:
            assert t.dim() == 1 or t.data_ptr() == x.data_ptr(), tuple(t.shape)          # [C] statistics, the source volume
            continue
        assert t.dtype == dt
        st = t.untyped_storage()
        if st.data_ptr() not in seen:
            seen.add(st.data_ptr())
            total += st.nbytes()
    model = sum(2 * r["z"].numel() + (2 * r["y"].numel() if r["y"] is not None else 0) for r in recs)
    model += 2 * sv["stem"]["col16"].numel() + 2 * sv["units"][0][0]["x"].numel()
    print(f"saved backbone state {prec}: {total} bytes, model {model}")
    assert abs(total - model) <= 0.01 * model
    del sv, state, recs

    tgt = torch.tensor([1, 0]).cuda()
    peaks = {}
    for storage in ("fp32", "16bit"):
        m = _slice_model(prec, storage)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        torch.nn.functional.cross_entropy(m(src), tgt).backward()
        torch.cuda.synchronize()
        peaks[storage] = torch.cuda.max_memory_allocated()
        del m
    print(f"peak memory of a step {prec}: {peaks}")
    assert peaks["16bit"] < peaks["fp32"]


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_bottleneck_model_and_plain_resnet_with_fc(prec):
    from mst.models import ResNet
    src = synth.synth_volume(SHAPE, 42).cuda()
    tgt = torch.tensor([1, 0]).cuda()
    m = _slice_model(prec, "16bit", model=50, seed=7)
    loss = torch.nn.functional.cross_entropy(m(src[:, :, :2]), tgt)
    loss.backward()
    assert bool(torch.isfinite(loss)) and all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in m.parameters())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = ResNet(in_ch=3, out_ch=2, spatial_dims=2, pretrained=False, model=18, train_precision=prec, train_storage="16bit")
    m.load_state_dict(synth.synth_resnet_state_dict(5, 18, 2, slice_trans=False, fc_out=2), strict=True)
    m = m.cuda().train()
    x = torch.from_numpy(synth.hash_normal((4, 3, 64, 96), 6, 1)).cuda()
    out = m(x)
    assert out.shape == (4, 2) and out.dtype == torch.float32
    torch.nn.functional.cross_entropy(out, torch.tensor([1, 0, 1, 0]).cuda()).backward()
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in m.parameters())
    assert float(m.model.conv1.weight.grad.abs().sum()) > 0


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------

def _step(build, src, tgt, autocast=None, scaler=None, opt=False):
    """One step from a fresh model; the forward inside the autocast region (if any), backward() outside it."""
    m = build()
    o = torch.optim.SGD(m.parameters(), lr=1e-3) if opt else None
    before = {k: p.detach().clone() for k, p in m.named_parameters()} if opt else None
    if autocast is None:
        logits = m(src)
    else:
        with torch.autocast("cuda", dtype=autocast):
            logits = m(src)
    assert logits.dtype == torch.float32
    loss = torch.nn.functional.cross_entropy(logits, tgt)
    if scaler is None:
        loss.backward()
    else:
        scaler.scale(loss).backward()
        scaler.unscale_(o)
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    if opt:
        (scaler.step(o) if scaler is not None else o.step())
    stats = {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k}
    return logits.detach().clone(), grads, stats, m, before


def test_two_16_bit_storage_steps_are_bit_identical_under_the_determinism_flag():
    src = synth.synth_volume(SHAPE, 42).cuda()
    tgt = torch.tensor([1, 0]).cuda()
    with _deterministic():
        a = _step(lambda: _slice_model("fp16", "16bit"), src, tgt)
        b = _step(lambda: _slice_model("fp16", "16bit"), src, tgt)
    assert torch.equal(a[0], b[0])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


# ---- 7. autocast -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_a_defaulted_model_follows_the_autocast_region(prec, monkeypatch):
    from mst import train_resnet as T
    monkeypatch.delenv("MST_TRAIN_PRECISION", raising=False)
    monkeypatch.delenv("MST_RESNET_TRAIN_STORAGE", raising=False)
    dt = DT[prec]
    src = synth.synth_volume(SHAPE, 42).cuda()
    B, _, D, H, W = SHAPE
    x = src.float().reshape(B * D, H, W, 1).contiguous()

    def saved(m, region):
        with torch.no_grad(), (torch.autocast("cuda", dtype=dt) if region else contextlib.nullcontext()):
            out, sv = T.forward_train(m, x, True, B, D, None)
        assert out.dtype == torch.float32
        recs = [sv["stem"]] + [r for unit in sv["units"] for r in unit if r is not None]
        return sv, recs

    m = _slice_model()
    assert m.train_precision == "fp32" and m._train_precision_given is False
    sv, recs = saved(m, True)
    assert sv["mp"] == dt and sv["storage"] == "fp32" and all(r["mp"] == dt for r in recs)      # train_storage is never inferred
    sv, recs = saved(m, False)
    assert sv["mp"] is None and all(r["mp"] is None for r in recs)
    sv, recs = saved(_slice_model("fp32"), True)                                               # an explicit value is never overridden
    assert sv["mp"] is None and all(r["mp"] is None for r in recs)
    monkeypatch.setenv("MST_TRAIN_PRECISION", "fp32")
    sv, recs = saved(_slice_model(), True)
    assert sv["mp"] is None and all(r["mp"] is None for r in recs)
    monkeypatch.delenv("MST_TRAIN_PRECISION")
    # a whole step: the forward inside the region, backward() after it has ended -- the explicit step bit for bit
    tgt = torch.tensor([1, 0]).cuda()
    with _deterministic():
        inside = _step(_slice_model, src, tgt, autocast=dt)
        explicit = _step(lambda: _slice_model(prec), src, tgt)
    assert torch.equal(inside[0], explicit[0])
    for k in inside[1]:
        assert torch.equal(inside[1][k], explicit[1][k]), k


def test_grad_scaler_step_under_fp16_autocast(monkeypatch):
    """One torch.amp.GradScaler step of a defaulted model under fp16 autocast: finite gradients after unscale_, and the optimiser step
    is taken (GradScaler skips it when a gradient overflowed).  dz is rounded to fp16 unscaled by the step itself, so the scaler's factor
    multiplies it: the initial scale is 2^10, not the 2^16 default a real run backs off from within its first steps."""
    monkeypatch.delenv("MST_TRAIN_PRECISION", raising=False)
    src = synth.synth_volume(SHAPE, 42).cuda()
    tgt = torch.tensor([1, 0]).cuda()
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    _, grads, _, m, before = _step(_slice_model, src, tgt, autocast=torch.float16, scaler=scaler, opt=True)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    moved = [k for k, p in m.named_parameters() if not torch.equal(p.detach(), before[k])]
    assert len(moved) > 0.9 * len(before), (len(moved), len(before))
