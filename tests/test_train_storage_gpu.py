"""train_storage='16bit' of the DINOv2 training step (csrc/k_train16.hip, the 16-bit instantiations of the row kernels of csrc/k_train.hip and csrc/k_colsum.hip,
the 16-bit-output forms of csrc/k_attn16_train.hip) and the
autocast rule of train_precision: every new entry point against the existing fp32 entry points on the upcast inputs and against fp64
torch, the step against the fp32 step and the parent's flash step, the memory the saved state takes, determinism, autocast."""

import contextlib

import pytest
import torch

from mst import hip, synth, train
from test_attn_train_gpu import BWD_SHAPES, DT, FWD_SHAPES, _compare, _dino, _dino_reg, _grads, _qkv16

pytestmark = pytest.mark.gpu

ROWS = [1, 5, 257, 1030]
COLS = [384, 768]
ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}                                    # one unit in the last place of T, relative


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


@contextlib.contextmanager
def _deterministic(on=True):
    prev, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn)


# ---- A1: residual + LayerScale + LayerNorm ------------------------------------------------------------------------------------------

def _ln_error(x_out, y, w, b, eps=1e-6):
    """Worst error of y against the fp64 LayerNorm of x_out, relative to |want|, after 1e-6 absolute is taken off."""
    xo = x_out.double()
    mu = xo.mean(1, keepdim=True)
    var = (xo - mu).square().mean(1, keepdim=True)
    want = (xo - mu) / (var + eps).sqrt() * w.double() + b.double()
    return float(((y.double() - want).abs() - 1e-6).clamp_min(0).div(want.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_residual_layernorm16_against_fp64(rows, cols, prec):
    """x_out within one fp32 ulp of x_in + gamma * float(br) in fp64 (the kernel rounds once); y within one ulp of T (+ 1e-6 absolute) of
    the fp64 LayerNorm of that x_out.  The y == NULL and gamma == NULL forms; poisoned outputs are fully written."""
    g = _gen(rows * 7 + cols)
    T = DT[prec]
    x_in = torch.randn(rows, cols, device="cuda", generator=g) * 3
    br = (torch.randn(rows, cols, device="cuda", generator=g) * 2).to(T)
    gamma = torch.randn(cols, device="cuda", generator=g) * 0.5
    w = 1 + 0.2 * torch.randn(cols, device="cuda", generator=g)
    b = 0.2 * torch.randn(cols, device="cuda", generator=g)
    x_out, y = hip.residual_layernorm16(x_in, br, gamma, w, b, 1e-6)
    assert x_out.dtype == torch.float32 and y.dtype == T
    want_x = x_in.double() + gamma.double() * br.double()
    ex = float(((x_out.double() - want_x).abs() / want_x.abs().clamp_min(1e-300)).max())
    ey = _ln_error(x_out, y, w, b)
    print(f"residual_layernorm16 {prec} [{rows}, {cols}]: x_out {ex / 2 ** -23:.2f} fp32 ulp, y {ey / ULP[prec]:.2f} ulp of T")
    assert ex <= 2.0 ** -23, ex
    assert ey <= ULP[prec], ey
    # caller-given poisoned outputs: every element written, the same bits
    px = torch.full_like(x_in, float("nan"))
    py = torch.full_like(br, float("nan"))
    hip.residual_layernorm16(x_in, br, gamma, w, b, 1e-6, x_out=px, y=py)
    assert torch.equal(_bits(px), _bits(x_out)) and torch.equal(_bits(py), _bits(y))
    # y == NULL: the residual alone
    x_only, none = hip.residual_layernorm16(x_in, br, gamma, None, None, 1e-6)
    assert none is None and torch.equal(_bits(x_only), _bits(x_out))
    # gamma == NULL: no LayerScale
    x_ng, y_ng = hip.residual_layernorm16(x_in, br, None, w, b, 1e-6)
    want_ng = x_in.double() + br.double()
    assert float(((x_ng.double() - want_ng).abs() / want_ng.abs().clamp_min(1e-300)).max()) <= 2.0 ** -23
    assert _ln_error(x_ng, y_ng, w, b) <= ULP[prec]


def test_residual_layernorm16_rejects_bad_arguments():
    x = torch.zeros(4, 388, device="cuda")                                       # 388 = 4 * 97: not a multiple of 8
    with pytest.raises(RuntimeError, match="multiple of 8"):
        hip.residual_layernorm16(x, x.half(), None, None, None, 1e-6)
    with pytest.raises(TypeError):
        hip.residual_layernorm16(x, x, None, None, None, 1e-6)


# ---- A2: activation -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("n", [5, 8, 1 * 1536, 5 * 3072, 257 * 1536 + 3, 1030 * 3072, 1030 * 1536 + 7])
def test_act16_is_the_fp32_entry_point_on_the_upcast_input(n, prec):
    """mst_act_fwd16(h) == T(mst_act_fwd(float(h))) and mst_act_bwd16(h, dy) == mst_act_bwd(float(h), dy), bit for bit, at the hidden
    sizes 4E of rows x {384, 768} and at counts with a ragged tail (n % 8 != 0; n may be any positive count)."""
    g = _gen(n % 9973)
    T = DT[prec]
    h = (torch.randn(n, device="cuda", generator=g) * 2.5).to(T)
    dy = torch.randn(n, device="cuda", generator=g)
    for kind in (0, 1):
        assert torch.equal(_bits(hip.act_fwd16(h, kind)), _bits(hip.act_fwd(h.float(), kind).to(T)))
        assert torch.equal(_bits(hip.act_bwd16(h, dy.clone(), kind)), _bits(hip.act_bwd(h.float(), dy.clone(), kind)))


# ---- A3: LayerScale gradient with a 16-bit factor --------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS + [4112])                                  # 4112 rows: more than one row block (the slab path)
def test_colsum_b16_ordered_and_atomic(rows, cols, prec):
    """Ordered form: the bits of mst_colsum_ordered on float(b).  Atomic form: within rows * 2^-24 * sum |a b| per column of the fp64 sum
    (every partial sum is at most sum |a b|, each of the < rows additions rounds once).  rows == 257: operands that are column blocks of
    wider matrices (row stride cols + 64)."""
    g = _gen(rows + cols)
    T = DT[prec]
    wide = cols + 64 if rows == 257 else cols
    a = torch.randn(rows, wide, device="cuda", generator=g)[:, :cols]
    b = torch.randn(rows, wide, device="cuda", generator=g).to(T)[:, :cols]
    start = torch.randn(cols, device="cuda", generator=g)                        # the entry points add to `out`
    with _deterministic():
        got = hip.colsum(a, start.clone(), b=b)
        ref = hip.colsum(a, start.clone(), b=b.float())
        assert torch.equal(_bits(got), _bits(ref))
        assert torch.equal(_bits(hip.colsum(a, start.clone(), b=b)), _bits(got))
    with _deterministic(False):
        got = hip.colsum(a, torch.zeros(cols, device="cuda"), b=b)
    prod = a.double() * b.double()
    err = (got.double() - prod.sum(0)).abs()
    bound = rows * 2.0 ** -24 * prod.abs().sum(0)
    print(f"colsum_b16 {prec} [{rows}, {cols}]: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


# ---- A4: attention with a 16-bit output -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("n,heads,N", FWD_SHAPES)
def test_attention_fwd16_is_the_rounded_fp32_output(prec, n, heads, N):
    qkv = _qkv16(n, heads, N, DT[prec], 1000 + N + heads)
    out32, lse32 = hip.attention_train_fwd(qkv, n, N, heads)
    out16, lse16 = hip.attention_train_fwd(qkv, n, N, heads, out_dtype=DT[prec])
    assert out16.dtype == DT[prec]
    assert torch.equal(_bits(out16), _bits(out32.to(DT[prec])))
    assert torch.equal(_bits(lse16), _bits(lse32))


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("n,heads,N", BWD_SHAPES)
def test_attention_bwd16_is_the_fp32_entry_point_on_the_upcast_output(prec, n, heads, N):
    qkv = _qkv16(n, heads, N, DT[prec], 2000 + N + heads)
    dout = torch.randn(n * N, heads * 64, device="cuda", generator=_gen(7 + N))
    out16, lse = hip.attention_train_fwd(qkv, n, N, heads, out_dtype=DT[prec])
    got = hip.attention_train_bwd(qkv, out16, dout, lse, n, N, heads, dq_scale=0.125)
    ref = hip.attention_train_bwd(qkv, out16.float(), dout, lse, n, N, heads, dq_scale=0.125)
    assert torch.equal(_bits(got), _bits(ref))
    assert torch.equal(_bits(hip.attention_train_bwd(qkv, out16, dout, lse, n, N, heads, dq_scale=0.125)), _bits(got))


# ---- A5: transposed operand image ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("rows,cols,rows_pad", [(1000, 384, 1024), (257, 1536, 320)])
def test_transpose16(rows, cols, rows_pad, prec):
    x = torch.randn(rows, cols, device="cuda", generator=_gen(rows)).to(DT[prec])
    want = torch.zeros(cols, rows_pad, dtype=DT[prec], device="cuda")
    want[:, :rows] = x.t()
    out = hip.transpose16(x, rows_pad=rows_pad)
    assert out.shape == (cols, rows_pad) and torch.equal(_bits(out), _bits(want))
    assert torch.equal(_bits(out), _bits(hip.cvt16(x.float(), DT[prec], transpose=True, rows_pad=rows_pad)))


# ---- the training step --------------------------------------------------------------------------------------------------------------

def _with_storage(build_of, storage):
    """build_of(prec, attn[, size]) -> builder, as the STEP_CASES of test_attn_train_gpu; the built model gets train_storage = storage."""
    def make(*args):
        inner = build_of(*args)

        def build():
            m = inner()
            m.train_storage = storage
            return m
        return build
    return make


# (builder, size, precision, bars against the fp32 step: per parameter (and logits), global rel-L2) -- the project's bars of
# test_mixed_precision_step_gradients_against_the_fp32_step / test_flash_step_gradients_against_the_fp32_and_stored_steps.
# Measured on the MI355X, logits / worst parameter / global, '16bit' vs fp32 (flash with fp32 storage vs fp32) [ratio]:
#   s_fp16       1.25e-3 / 5.51e-3 / 3.92e-3   (7.10e-4 / 5.57e-3 / 4.00e-3)   [1.76 0.99 0.98]
#   s_bf16       8.52e-3 / 3.52e-2 / 2.53e-2   (1.45e-2 / 3.48e-2 / 2.71e-2)   [0.59 1.01 0.94]
#   reg261_fp16  2.61e-3 / 5.07e-3 / 3.81e-3   (2.32e-3 / 5.47e-3 / 3.91e-3)   [1.12 0.93 0.98]
#   vitb_fp16    1.46e-3 / 5.07e-3 / 3.86e-3   (1.10e-3 / 4.52e-3 / 3.29e-3)   [1.33 1.12 1.17]
#   s_fp16 at 1 x 48 x 224^2 (test_16bit_storage_step_above_12288_tokens):
#                6.37e-5 / 7.10e-3 / 4.96e-3   (4.83e-4 / 4.11e-2 / 1.40e-2)   [0.13 0.17 0.35]
#   d source (test_16bit_storage_source_gradient_and_frozen_model): 5.70e-3 (5.77e-3) [0.99]
#   GradScaler step vs the unscaled fp16 step: 0 / 2.96e-3 / 2.20e-3
#   saved block state 40.06 E bytes per token (80.06 E with fp32 storage); peak at 1 x 8 x 518^2 bf16 6.03 -> 4.06 GiB
STEP_CASES = {
    "s_fp16": (_dino, "s", "fp16", (1e-2, 8e-3)),
    "s_bf16": (_dino, "s", "bf16", (1.3e-1, 7e-2)),
    "reg261_fp16": (_dino_reg, None, "fp16", (1e-2, 8e-3)),
    "vitb_fp16": (_dino, "b", "fp16", (1e-2, 8e-3)),
}
SHAPE = (1, 1, 4, 224, 224)


def _check_against_references(name, got, full, flash, bars):
    """Errors of `got` against the fp32 step: below the project's bars, and at most 2x the errors of the flash / fp32-storage step against
    the same fp32 step (the new roundings are of the operands' own size at about 1.5x as many sites; 2x is the project's margin)."""
    d, w, g = _compare(got, full)
    dp, wp, gp = _compare(flash, full)
    print(f"{name}: 16bit vs fp32 logits {d:.2e} worst {w:.2e} global {g:.2e} | flash vs fp32 logits {dp:.2e} worst {wp:.2e} global {gp:.2e} | "
          f"ratios {d / dp:.2f} {w / wp:.2f} {g / gp:.2f}")
    assert d < bars[0] and w < bars[0] and g < bars[1], (d, w, g)
    assert d <= 2 * dp and w <= 2 * wp and g <= 2 * gp, ((d, dp), (w, wp), (g, gp))


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_16bit_storage_step_gradients_against_the_fp32_and_flash_steps(case):
    """train_storage='16bit' at (1, 1, 4, 224, 224): logits and every parameter gradient against the fp32 step (fp16 1e-2 per parameter /
    8e-3 global rel-L2, bf16 1.3e-1 / 7e-2), each error at most 2x that of the flash step with fp32 storage against the same fp32 step."""
    mk, size, prec, bars = STEP_CASES[case]
    mk16 = _with_storage(mk, "16bit")
    build = (lambda p, a: mk16(p, a, size)) if size else mk16
    src = synth.synth_volume(SHAPE, 3).cuda()
    tgt = torch.tensor([1]).cuda()
    ref = (lambda p, a: mk(p, a, size)) if size else mk
    full, flash = _grads(ref("fp32", "stored"), src, tgt), _grads(ref(prec, "flash"), src, tgt)
    _check_against_references(case, _grads(build(prec, "flash"), src, tgt), full, flash, bars)


def test_16bit_storage_step_above_12288_tokens():
    """(1, 1, 48, 224, 224): 12,336 token rows, the weight gradients through the transposed operand images (mst_transpose16 of the saved
    16-bit activations) and the split-K GEMM."""
    shape = (1, 1, 48, 224, 224)
    src = synth.synth_volume(shape, 3).cuda()
    tgt = torch.tensor([1]).cuda()
    full = _grads(_dino("fp32", "stored", "s"), src, tgt)
    flash = _grads(_dino("fp16", "flash", "s"), src, tgt)
    got = _grads(_with_storage(_dino, "16bit")("fp16", "flash", "s"), src, tgt)
    _check_against_references("s_fp16 48 slices", got, full, flash, (1e-2, 8e-3))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def test_16bit_storage_source_gradient_and_frozen_model():
    """source.requires_grad_(): d source of the 16-bit storage step is present, finite and within 2x the flash step's error against the
    fp32 step; a frozen model's source-only backward works and gives that gradient."""
    tgt = torch.tensor([1]).cuda()
    res = {}
    for name, build in (("fp32", _dino("fp32", "stored", "s")), ("flash", _dino("fp16", "flash", "s")),
                        ("16bit", _with_storage(_dino, "16bit")("fp16", "flash", "s"))):
        m = build().cuda().train()
        src = synth.synth_volume(SHAPE, 3).cuda().requires_grad_()
        torch.nn.functional.cross_entropy(m(src), tgt).backward()
        assert src.grad is not None and src.grad.shape == src.shape and bool(torch.isfinite(src.grad).all())
        res[name] = src.grad.clone()
        if name == "16bit":
            m.requires_grad_(False)
            frozen = synth.synth_volume(SHAPE, 3).cuda().requires_grad_()
            torch.nn.functional.cross_entropy(m(frozen), tgt).backward()
            assert frozen.grad is not None and bool(torch.isfinite(frozen.grad).all()) and _rel(frozen.grad, src.grad) < 1e-5
    e16, efl = _rel(res["16bit"], res["fp32"]), _rel(res["flash"], res["fp32"])
    print(f"d source: 16bit vs fp32 {e16:.2e}, flash vs fp32 {efl:.2e}, ratio {e16 / efl:.2f}")
    assert e16 <= 2 * efl, (e16, efl)


def test_16bit_storage_step_is_deterministic_under_the_flag():
    """torch.use_deterministic_algorithms(True): two steps on the same state and input give bit-identical logits and gradients (the
    LayerScale gradients take mst_colsum_b16_ordered)."""
    src = synth.synth_volume(SHAPE, 3).cuda()
    tgt = torch.tensor([1]).cuda()
    build = _with_storage(_dino_reg, "16bit")("fp16", "flash")                   # the register model has LayerScale
    with _deterministic():
        m = build().cuda().train()
        runs = []
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            logits = m(src)
            torch.nn.functional.cross_entropy(logits, tgt).backward()
            runs.append((logits.detach().clone(), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert set(runs[0][1]) == set(runs[1][1]) and len(runs[0][1]) > 100
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


# ---- memory ---------------------------------------------------------------------------------------------------------------------------

def _reachable_bytes(obj, seen):
    if torch.is_tensor(obj):
        if obj.is_cuda and obj.data_ptr() not in seen:
            seen[obj.data_ptr()] = obj.numel() * obj.element_size()
    elif isinstance(obj, dict):
        for v in obj.values():
            _reachable_bytes(v, seen)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _reachable_bytes(v, seen)
    return sum(seen.values())


def test_saved_state_of_the_blocks_is_40E_bytes_per_token():
    """What forward_train keeps in sv["blocks"] at (1, 1, 2, 224, 224): at most 1.02 x 12 x (40 E M + the log-sum-exp) unique device bytes
    in the 16-bit storage mode; the same walk on the flash mode with fp32 storage sees at least 12 x 66 E M."""
    src = synth.synth_volume((1, 1, 2, 224, 224), 3).cuda()
    n, heads, N, E = 2, 6, 257, 384
    M = n * N
    seen = {}
    for storage in ("16bit", "fp32"):
        m = _with_storage(_dino, storage)("fp16", "flash", "s")().cuda().train()
        with torch.no_grad():
            _, sv = train.forward_train(m, src, None, False)
        torch.cuda.synchronize()
        seen[storage] = _reachable_bytes(sv["blocks"], {})
        if storage == "16bit":
            assert all(not s["x16"] for s in sv["blocks"])
            assert sv["mp"] is torch.float16 and sv["storage16"] is True
        del sv, m
    print(f"saved block state: 16bit {seen['16bit']} B ({seen['16bit'] / (12 * E * M):.2f} E per token), fp32 storage {seen['fp32']} B "
          f"({seen['fp32'] / (12 * E * M):.2f} E per token)")
    assert seen["16bit"] <= 1.02 * 12 * (40 * E * M + 4 * n * heads * N)
    assert seen["fp32"] >= 12 * 66 * E * M


def test_16bit_storage_lowers_the_peak_of_a_step():
    """Peak memory of one bf16 step at (1, 1, 8, 518, 518), M = 8 x 1370 rows: below the flash / fp32-storage peak by at least
    0.75 x 12 x M x 26 E bytes (26 E = 66 E - 40 E of the two saved-state tables)."""
    src = synth.synth_volume((1, 1, 8, 518, 518), 5).cuda()
    tgt = torch.tensor([0]).cuda()
    peaks = {}
    for storage in ("fp32", "16bit"):
        m = _with_storage(_dino, storage)("bf16", "flash", "s")().cuda().train()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        torch.nn.functional.cross_entropy(m(src), tgt).backward()
        torch.cuda.synchronize()
        peaks[storage] = torch.cuda.max_memory_allocated()
        del m
        torch.cuda.empty_cache()
    need = 0.75 * 12 * 8 * 1370 * 26 * 384
    print(f"peak GiB: fp32 storage {peaks['fp32'] / 2**30:.2f}, 16bit {peaks['16bit'] / 2**30:.2f}; saved {(peaks['fp32'] - peaks['16bit']) / 1e9:.2f} GB, "
          f"need {need / 1e9:.2f} GB")
    assert peaks["fp32"] - peaks["16bit"] >= need


# ---- autocast -----------------------------------------------------------------------------------------------------------------------

def _plain(**kw):
    from mst.models import DinoV2ClassifierSlice

    def build():
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, **kw)
        m.load_state_dict(synth.synth_state_dict("s", 0))
        return m
    return build


def _step(build, src, tgt, autocast=None, scaler=None):
    """One step; the forward inside the autocast region (if any), backward() outside it."""
    m = build().cuda().train()
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
        opt = torch.optim.SGD(m.parameters(), lr=0.0)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
    return logits.detach(), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}


def _same_bits(a, b):
    assert torch.equal(a[0], b[0])
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_a_defaulted_model_follows_the_autocast_region(prec, monkeypatch):
    """No train_precision keyword, no MST_TRAIN_PRECISION: inside torch.autocast('cuda', T) the step is the explicit train_precision=T
    step bit for bit (deterministic flag on, backward() outside the region); the attribute still reads 'fp32' and outside a region the
    model runs the fp32 step."""
    monkeypatch.delenv("MST_TRAIN_PRECISION", raising=False)
    src = synth.synth_volume((1, 1, 2, 224, 224), 3).cuda()
    tgt = torch.tensor([1]).cuda()
    with _deterministic():
        explicit = _step(_plain(train_precision=prec), src, tgt)
        inside = _step(_plain(), src, tgt, autocast=DT[prec])
        outside = _step(_plain(), src, tgt)
        full = _step(_plain(train_precision="fp32"), src, tgt)
    assert _plain()().train_precision == "fp32"
    _same_bits(inside, explicit)
    _same_bits(outside, full)
    assert any(not torch.equal(inside[1][k], full[1][k]) for k in full[1])


def test_the_resolver_inside_an_autocast_region(monkeypatch):
    """train_mode.resolve alone (torch opens no CUDA autocast region without a device, so this is not a CPU test): a defaulted model takes
    the region's type and nothing else, a model built with train_precision='fp32' does not."""
    from mst.train_mode import TrainMode, resolve
    for name in ("MST_TRAIN_PRECISION", "MST_TRAIN_ATTENTION", "MST_TRAIN_STORAGE"):
        monkeypatch.delenv(name, raising=False)
    defaulted, given = _plain()(), _plain(train_precision="fp32")()
    with torch.autocast("cuda", torch.bfloat16):
        assert resolve(defaulted) == TrainMode(mp=torch.bfloat16, flash=False, storage16=False)
        assert resolve(given).mp is None
    assert resolve(defaulted).mp is None                                           # nothing changes outside a region


def test_an_explicit_fp32_model_ignores_the_autocast_region(monkeypatch):
    monkeypatch.delenv("MST_TRAIN_PRECISION", raising=False)
    src = synth.synth_volume((1, 1, 2, 224, 224), 3).cuda()
    tgt = torch.tensor([1]).cuda()
    with _deterministic():
        outside = _step(_plain(train_precision="fp32"), src, tgt)
        inside = _step(_plain(train_precision="fp32"), src, tgt, autocast=torch.float16)
        monkeypatch.setenv("MST_TRAIN_PRECISION", "fp32")
        by_env = _step(_plain(), src, tgt, autocast=torch.float16)
    _same_bits(inside, outside)
    _same_bits(by_env, outside)


def test_grad_scaler_step_under_autocast(monkeypatch):
    """One torch.amp.GradScaler step of a defaulted model under fp16 autocast (scale(loss).backward(); unscale_(opt)): finite gradients,
    within the fp16 bars (1e-2 per parameter, 8e-3 global rel-L2) of the unscaled explicit fp16 step."""
    monkeypatch.delenv("MST_TRAIN_PRECISION", raising=False)
    src = synth.synth_volume((1, 1, 2, 224, 224), 3).cuda()
    tgt = torch.tensor([1]).cuda()
    plain = _step(_plain(train_precision="fp16"), src, tgt)
    scaled = _step(_plain(), src, tgt, autocast=torch.float16, scaler=torch.amp.GradScaler("cuda"))
    assert all(bool(torch.isfinite(g).all()) for g in scaled[1].values())
    d, w, g = _compare(scaled, plain)
    print(f"GradScaler step vs unscaled fp16 step: logits {d:.2e} worst {w:.2e} global {g:.2e}")
    assert d < 1e-2 and w < 1e-2 and g < 8e-3, (d, w, g)
