"""The 16-bit DINOv2 training step held, stage by stage, to float64 on its own record (tests/mixed_audit.py), and `_Grads.lin_bwd` called
directly on every route it has."""
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
LIN_RUNS = ([("fallback", s, x) for s in FALLBACK for x in ("fp32", "T")]
            + [("wgrad", s, x) for s in WGRAD for x in ("fp32", "fp32+X16", "fp32+badX16", "T")]
            + [("splitk", s, x) for s in SPLITK for x in ("fp32", "T")])


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


def _check_lin(G, lin, dX, ref, what):
    got = {"dW": G.by_param[id(lin.weight)], "db": G.by_param[id(lin.bias)], "dX": dX}
    errs = {k: float((got[k].double() - r).abs().max() / r.abs().max()) for k, r in zip(("dW", "db", "dX"), ref)}
    print(f"{what}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert all(v.dtype == torch.float32 for v in got.values())
    assert max(errs.values()) <= A.BAR, errs
    return got


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("route,shape,xform", LIN_RUNS, ids=[f"{r}-{'x'.join(map(str, s))}-{x}" for r, s, x in LIN_RUNS])
def test_lin_bwd_routes(route, shape, xform, prec):
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
    G = _Grads(T)
    full = _check_lin(G, lin, G.lin_bwd(dY, Xin, lin, **kw), ref, f"{route} {shape} {xform} {prec}")
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
                assert float((t - full[k]).abs().max()) <= A.BAR * scale, (needed, need_dx, k)


@pytest.mark.parametrize("M,sp", [(63, 1), (130, 2), (131, 1), (1024, 16)])
def test_fp32_dw_split(M, sp):
    """The fp32 step's `_dw` (mp None): one product or `sp` row slabs reduced by mst_colsum, against float64."""
    from mst.train import _Grads
    N = K = 128
    assert next((d for d in (16, 8, 4, 2) if M % d == 0 and M // d >= 64), 1) == sp
    dY, X, lin = _operands(M, N, K, 3 + M)
    G = _Grads(None)
    _check_lin(G, lin, G.lin_bwd(dY, X, lin), _lin_reference(dY, X, lin.weight, None), f"fp32 _dw M={M} sp={sp}")
