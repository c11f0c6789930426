"""The 16-bit DINOv2 training step held, stage by stage, to float64 on its own record (tests/mixed_audit.py), and `_Grads.lin_bwd` called
directly on every route it has."""
import contextlib
import types

import pytest
import torch

import mixed_audit as A

pytestmark = pytest.mark.gpu

BLOCK_RUNS = A.RUNS      # the cases, what each one reaches and what it measured on the MI355X: the table above CASES in tests/mixed_audit.py


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("case,storage,attn", BLOCK_RUNS, ids=["-".join(r) for r in BLOCK_RUNS])
def test_block_audit(case, storage, attn, prec, monkeypatch):
    """Every saved tensor, every gradient of every block, dx0, the token stage's gradients and d volume of one recorded step against the
    float64 segments (bars: tests/mixed_audit.py); `hip_step` asserts the xn / x0 hand-off by identity."""
    rec = A.hip_step(case, prec, storage, attn, monkeypatch)
    res = A.audit(rec, case, prec, storage, attn)
    print(f"{case} {prec} {storage} {attn}: {A.worst(res)}")
    bad = A.failures(res, prec, storage, A.BAR)
    assert not bad, f"{len(bad)} above their bar: " + "; ".join(bad[:12])


@pytest.mark.parametrize("storage", ["fp32", "16bit"])
def test_swiglu_width_off_the_16_bit_tiles_is_refused(storage, monkeypatch):
    """E = 128 with SwiGLU hidden 344 (w12: N = 688, w3: K = 344) would put two fallback `lin_bwd` calls beside two 16-bit ones in one
    block, but the 16-bit forward refuses the width with a clean error, so no backward route is ever chosen for it."""
    with pytest.raises(RuntimeError, match="gemm16: N=688 must be a multiple of 128"):
        A.hip_step(A.REFUSED, "bf16", storage, "flash", monkeypatch)
    torch.cuda.synchronize()


# ---- _Grads.lin_bwd on its own --------------------------------------------------------------------------------------------------------
# (M, N, K) per route.  Measured on the MI355X, worst max |d| / max |ref| of dW / db / dX over the shapes, X forms and both precisions
# (bar 1e-5):   fallback 3.7e-7 / 1.5e-7 / 1.2e-6    conv_wgrad 1.7e-7 / 1.7e-7 / 2.7e-7    split-K 2.1e-7 / 6.4e-7 / 2.9e-7
#               fp32 `_dw` split (mp None) 3.6e-7 / 1.3e-7 / 4.1e-7
FALLBACK = [(63, 128, 128), (84, 688, 128), (84, 128, 344)]
WGRAD = [(64, 128, 128), (84, 384, 128), (1000, 128, 256)]
SPLITK = [(12289, 128, 128), (12352, 256, 128)]
# The weight shapes of ViT-L (fc1, fc2) and ViT-g (w12, w3): N * K from 4.2 M to 12.6 M, so the partial products that mst_colsum reduces
# are wider than the 65,535 column blocks one gridDim.y takes.  Smallest M per route: 300 is two conv_wgrad splits at these tile counts
# (hip.conv_wgrad: min(2048 // tiles, (M + 255) // 256) = 2), 12,352 the split-K route (two splits at 256 tiles; ONE at the 768 and 384
# tiles of ViT-g, which still goes through mst_colsum with one row); 130 and 1024 the fp32 `_dw` with 2 and 16 slabs.
WIDE = [(4096, 1024), (1024, 4096), (8192, 1536), (1536, 4096)]
WIDE_M = {"wgrad": 300, "splitk": 12352}
WIDE_RUNS = [(r, (M, N, K), x) for r, M in WIDE_M.items() for N, K in WIDE for x in ("fp32", "T")]
# The bar at these shapes.  A.BAR = 1e-5 is ten times the fp32 stand-in's distance from float64 at widths up to 688.  Measured on the MI355X
# at the shapes above, the stand-in (torch's fp32 product of the SAME rounded operands against float64 -- a reference, never the kernel),
# worst over the four shapes and both types, dW / db / dX:   M = 300: 8.2e-7 / 1.8e-7 / 3.6e-6    M = 12,352: 5.75e-6 / 2.2e-7 / 4.4e-6
# Ten times 5.75e-6 is above A.BAR, so the wide cases -- and only they -- are held to WIDE_BAR = 10 x that noise.  The routes themselves,
# worst max |d| / max |ref| of dW / db / dX:   conv_wgrad 2.0e-7 / 1.5e-7 / 1.6e-6    split-K 1.9e-6 / 3.5e-7 / 1.4e-6
#   fp32 `_dw` split 3.1e-7 / 1.5e-7 / 4.4e-6   (0.08 of WIDE_BAR at the worst; all below A.BAR as well)
WIDE_BAR = 5.8e-5
LIN_RUNS = ([("fallback", s, x) for s in FALLBACK for x in ("fp32", "T")]
            + [("wgrad", s, x) for s in WGRAD for x in ("fp32", "fp32+X16", "fp32+badX16", "T")]
            + [("splitk", s, x) for s in SPLITK for x in ("fp32", "T")]
            + WIDE_RUNS)


def _operands(M, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dY = torch.randn(M, N, device="cuda", generator=g)
    X = torch.randn(M, K, device="cuda", generator=g)
    lin = types.SimpleNamespace(weight=torch.randn(N, K, device="cuda", generator=g) / K ** 0.5,
                                bias=torch.randn(N, device="cuda", generator=g))
    return dY, X, lin


def _lin_reference(dY, X, W, T):
    """float64 dW, db, dX on operands rounded to T as the 16-bit route rounds them (T None: the fp32 routes, nothing rounded)."""
    r = (lambda t: t.to(T).double()) if T is not None else (lambda t: t.double())
    return r(dY).t() @ r(X), dY.double().sum(0), r(dY) @ r(W)


def _spy_on_colsum(monkeypatch, width):
    """hip.colsum as it is, with the row count of every call on `width` columns (the reduction of a weight's partial products) noted."""
    from mst import hip
    rows, real = [], hip.colsum

    def colsum(a, out, b=None):
        if a.shape[1] == width:
            rows.append(a.shape[0])
        return real(a, out, b)
    monkeypatch.setattr(hip, "colsum", colsum)
    return rows


def _wide_splits(route, N, K):
    tiles = (N // 128) * (K // 128)
    return 2 if route == "wgrad" else {256: 2, 768: 1, 384: 1}[tiles]


@contextlib.contextmanager
def _deterministic(on):
    prev, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(on)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(prev, warn_only=warn)


def _bar(N, K):
    return WIDE_BAR if (N, K) in WIDE else A.BAR


def _check_lin(G, lin, dX, ref, what):
    got = {"dW": G.by_param[id(lin.weight)], "db": G.by_param[id(lin.bias)], "dX": dX}
    errs = {k: float((got[k].double() - r).abs().max() / r.abs().max()) for k, r in zip(("dW", "db", "dX"), ref)}
    print(f"{what}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert all(v.dtype == torch.float32 for v in got.values())
    assert max(errs.values()) <= _bar(*lin.weight.shape), errs
    return got


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("route,shape,xform", LIN_RUNS, ids=[f"{r}-{'x'.join(map(str, s))}-{x}" for r, s, x in LIN_RUNS])
def test_lin_bwd_routes(route, shape, xform, prec, monkeypatch):
    """dW, db and dX of `_Grads(mp).lin_bwd` against float64 on the operands rounded exactly as the route rounds them -- exact up to fp32
    accumulation, so the fp32-valued bar.  X forms: fp32, fp32 beside the forward's kept image X16 (which must be the one read: it is given
    another matrix's image), an X16 of the wrong shape or dtype (must be ignored), X saved in T.  Then the result subsets."""
    from mst import hip
    from mst.train import _Grads
    M, N, K = shape
    T = A.DT[prec]
    dY, X, lin = _operands(M, N, K, 11 + M + N + K)
    route16 = N % 128 == 0 and K % 128 == 0 and M >= 64
    assert route16 == (route != "fallback") and (M > 12288) == (route == "splitk")
    Xin, Xref, kw = X, X, {}
    if xform == "T":
        Xin = Xref = X.to(T)
    elif xform == "fp32+X16":
        other = torch.randn(M, K, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        kw["X16"], Xref = hip.cvt16(other, T), other
    elif xform == "fp32+badX16":
        bad_dtype = torch.bfloat16 if T == torch.float16 else torch.float16
        kw["X16"] = [torch.ones(M + 1, K, dtype=T, device="cuda"), torch.ones(M, K, dtype=bad_dtype, device="cuda")][(M // 4) % 2]
    ref = _lin_reference(dY, Xref.float(), lin.weight, T if route16 else None)
    splits = _spy_on_colsum(monkeypatch, N * K)
    G = _Grads(T)
    full = _check_lin(G, lin, G.lin_bwd(dY, Xin, lin, **kw), ref, f"{route} {shape} {xform} {prec}")
    if (N, K) in WIDE:                                   # the partial products of the weight, as many as the route's comment above says
        assert splits == [_wide_splits(route, N, K)], splits
    # result subsets: what is not asked for is absent, what is asked for is what the full call gave (the split routes sum their partials
    # with atomics while the deterministic flag is off: within the bar, not by bits)
    for needed, need_dx in (({id(lin.weight)}, True), ({id(lin.bias)}, True), (None, False), ({id(lin.weight)}, False)):
        G = _Grads(T, needed=needed)
        dX = G.lin_bwd(dY, Xin, lin, need_dx=need_dx, **kw)
        assert (dX is None) == (not need_dx)
        assert set(G.by_param) == (needed if needed is not None else {id(lin.weight), id(lin.bias)})
        for k, t in (("dW", G.by_param.get(id(lin.weight))), ("db", G.by_param.get(id(lin.bias))), ("dX", dX)):
            if t is not None:
                scale = float(full[k].abs().max())
                assert float((t - full[k]).abs().max()) <= _bar(N, K) * scale, (needed, need_dx, k)


DW_RUNS = [(63, 1, 128, 128), (130, 2, 128, 128), (131, 1, 128, 128), (1024, 16, 128, 128)] + [(M, sp, N, K) for M, sp in ((130, 2), (1024, 16)) for N, K in WIDE]


@pytest.mark.parametrize("M,sp,N,K", DW_RUNS, ids=[f"{M}-{sp}" + ("" if N == K == 128 else f"-{N}x{K}") for M, sp, N, K in DW_RUNS])
def test_fp32_dw_split(M, sp, N, K, monkeypatch):
    """The fp32 step's `_dw` (mp None): one product or `sp` row slabs reduced by mst_colsum, against float64.  At the weight shapes of
    ViT-L / g the slabs are [sp, N * K] with N * K past one gridDim.y of column blocks."""
    from mst.train import _Grads
    assert next((d for d in (16, 8, 4, 2) if M % d == 0 and M // d >= 64), 1) == sp
    dY, X, lin = _operands(M, N, K, 3 + M)
    splits = _spy_on_colsum(monkeypatch, N * K)
    G = _Grads(None)
    _check_lin(G, lin, G.lin_bwd(dY, X, lin), _lin_reference(dY, X, lin.weight, None), f"fp32 _dw M={M} sp={sp} {N}x{K}")
    assert splits == ([sp] if sp > 1 else [])


# ---- the same shapes on operands whose every product and sum is exact ----------------------------------------------------------------
def _exact_operands(M, N, K, seed):
    """Rank one, small integers: dY[m, n] = a[m] p[n], X[m, k] = b[m] q[k] with |a|, |b| <= 2 and 1 <= |p|, |q| <= 6.  Every operand
    element (|.| <= 12) is exact in bf16 and fp16, every product an integer of at most 144, and every partial sum of dW[n, k] =
    (sum_m a b) p[n] q[k] an integer below 4 M |p| |q| <= 144 * 12,352 < 2^24: exact in fp32 in ANY order, split or tiling.  p and q
    are random, so a tile or a column piece written to another place lands on other values."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ri = lambda n, lo, hi: torch.randint(lo, hi + 1, (n,), device="cuda", generator=g).float()
    sg = lambda n: torch.randint(0, 2, (n,), device="cuda", generator=g).float() * 2 - 1
    a, b = ri(M, -2, 2), ri(M, -2, 2)
    p, q = ri(N, 1, 6) * sg(N), ri(K, 1, 6) * sg(K)
    return a, b, p, q


# (route, M, N, K, prec, deterministic): every shape on every route with the flag off; on, for contrast, once per route
EXACT_RUNS = ([("fp32", M, N, K, None, False) for M in (130, 1024) for N, K in WIDE]
              + [(r, M, N, K, prec, False) for r, M in WIDE_M.items() for N, K in WIDE for prec in ("fp16", "bf16")]
              + [("fp32", 1024, *WIDE[0], None, True)] + [(r, M, *WIDE[0], "bf16", True) for r, M in WIDE_M.items()])


@pytest.mark.parametrize("route,M,N,K,prec,det", EXACT_RUNS,
                         ids=[f"{r}-{M}-{N}x{K}-{prec or 'fp32'}-{'deterministic' if det else 'atomic'}" for r, M, N, K, prec, det in EXACT_RUNS])
def test_lin_bwd_wide_weights_exact_integers(route, M, N, K, prec, det, monkeypatch):
    """dW = (sum_m a b) p q^T and db = (sum_m a) p BIT FOR BIT on all N x K outputs of the ViT-L / g weight shapes, on every route that
    reduces partial products with mst_colsum, X as fp32 and saved in T: every tile of every split and every column piece of the
    reduction lands where it should, with no 150-GFLOP reference.  The deterministic flag is off in all but the contrast cases: the arm
    that raised `colsum: cols=... out of range` before the atomic form walked its column blocks in pieces."""
    from mst.train import _Grads
    T = None if route == "fp32" else A.DT[prec]
    a, b, p, q = _exact_operands(M, N, K, M + N + K)
    dY, X = a[:, None] * p[None, :], b[:, None] * q[None, :]
    lin = types.SimpleNamespace(weight=torch.zeros(N, K, device="cuda"), bias=torch.zeros(N, device="cuda"))
    want_w = float((a.double() * b.double()).sum()) * p.double()[:, None] * q.double()[None, :]
    want_b = float(a.double().sum()) * p.double()
    assert 0 < float(want_w.abs().max()) < 2 ** 24
    splits = _spy_on_colsum(monkeypatch, N * K)
    with _deterministic(det):
        for Xin in ((X,) if T is None else (X, X.to(T))):
            splits.clear()
            G = _Grads(T)
            assert G.lin_bwd(dY, Xin, lin, need_dx=False) is None
            assert splits == [{130: 2, 1024: 16}[M] if route == "fp32" else _wide_splits(route, N, K)], splits
            dW, db = G.by_param[id(lin.weight)], G.by_param[id(lin.bias)]
            assert dW.dtype == torch.float32 and dW.shape == (N, K)
            wrong = dW.double() != want_w
            assert not bool(wrong.any()), f"{int(wrong.sum())} of {N * K} weight gradients differ; first at {torch.nonzero(wrong)[0].tolist()}"
            assert torch.equal(db.double(), want_b)


@pytest.mark.parametrize("route,M", list(WIDE_M.items()))
def test_lin_bwd_wide_weights_deterministic(route, M):
    """One run per route of the random operands under the flag (the ordered reduction, which had no column limit), at the same bar."""
    from mst.train import _Grads
    N, K = WIDE[0]
    T = torch.bfloat16
    dY, X, lin = _operands(M, N, K, 11 + M + N + K)
    with _deterministic(True):
        G = _Grads(T)
        _check_lin(G, lin, G.lin_bwd(dY, X, lin), _lin_reference(dY, X, lin.weight, T), f"{route} ({M}, {N}, {K}) deterministic")
