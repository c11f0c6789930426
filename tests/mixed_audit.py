"""Stage-by-stage float64 audit of the 16-bit DINOv2 training step (mst/train.py: `_block_fwd`, `_block_fwd_16`, `_Grads.lin_bwd`,
`_encoder_bwd` with a 16-bit train_precision) ON THE STEP'S OWN RECORD.

The whole-step comparisons with the fp32 step (tests/test_train_gpu.py, test_attn_train_gpu.py, test_train_storage_gpu.py) hold the
compounded rounding error of twelve blocks: 1e-2 per parameter in fp16, 1.3e-1 in bf16.  Here nothing compounds.

Forward.  Every tensor the step saved (x0, xn1, qkv16, a, lse, br1, x1, xn2, hpre / hact or x12 / h, br2; qkv and P of the 'stored' attention)
is recomputed in float64 from the SAVED tensor(s) before it, with the roundings mst/train.py and mst/train_mode.py document: a linear is
r(x) . r(W)^T + b (q columns times 0.125), rounded to T where the step writes T; LayerNorm, residual + LayerScale, GELU and SwiGLU are
float64 on the upcast input; x2 is the next block's x0.  The token stage and the final LayerNorm are fp32 ops: the oracle in float64.
Backward.  float64 autograd over the same graph, in which every saved tensor has the saved value (y_ref + (y_saved - y_ref).detach()) and a
linear's backward is dX = r(dY) . r(W), dW = r(dY)^T . r(x_saved), db = column sums of the unrounded dY -- on the fp32 fallback route
(N % 128, K % 128 or M < 64) nothing is rounded.  The dY of every `lin_bwd` call is recorded and treated like a saved tensor: the reference's
own dY is compared with it, the three products read the recorded one.  Without that a gradient that fp32 and float64 round to different
neighbours in T moves a weight gradient by an ulp of T times one row -- 2e-3 of its maximum in bf16, measured on the stand-in -- and no bar
below the old ones could hold; with it r(dY) is the same image on both sides and every product is exact up to fp32 accumulation.
The attention core is not modelled.  `attention_train_bwd` is recorded in the running step: its `da` is compared with the reference's, its
`dqkv` with float64 autograd of softmax(q k^T) v on the recorded qkv16 (dQ times 0.125) at BWD_BARS of tests/test_attn_train_gpu.py -- the
check that pins dq_scale and the argument order in situ -- and the reference goes on from the recorded dqkv.
The gradient of the embeddings reaches the CLS rows only; `hip_step` adds a dense term to the gradient entering the last block, so that
every token row weighs in every product of every block (a one-block encoder would otherwise feed proj, fc1 and fc2 four non-zero rows).

A helper module like tests/train_parity.py: the cases, the reference, a CPU stand-in of the HIP step (`standin_step`: the same segment
arithmetic chained in torch fp32, the same roundings, a record of the same layout) and the mutants over it.

Bars (tests/test_mixed_audit_cpu.py derives them from the stand-in alone, tests/test_mixed_audit_gpu.py holds the HIP step to them):
  fp32-valued results (fp32 saved tensors, every recorded dY, every gradient, dx0, d volume, da): max |d| <= BAR * max |ref| per tensor
      (train_parity.scaled_errors' metric).  BAR = 1e-5 = 10 x NOISE, the worst stand-in-against-float64 value over RUNS and both
      precisions (measured 9.7e-7): the rule of tests/train_parity.py, room for another, equally valid fp32 summation order, atomics included.
  tensors saved in T: at most SHARE = 1e-3 of a tensor's elements not bit-equal to r(ref), and every element within 1 ulp of T of r(ref)
      OR within BAR * max |ref| of ref.  The second alternative is what an fp32 result rounded once can promise: an fp32 accumulator is
      off by ~1e-7 of the LARGEST terms, an ulp of T shrinks with the element, so an output near zero (a sum that cancels) is several ulps
      of T from r(ref) however it is computed -- the stand-in's plain fp32 dot product put a qkv16 element 13 fp16 ulps off, the MI355X 4,
      and the fp32 GELU's 1 + erf below -4 a bf16 hact of 1e-7 13,000 ulps off on both.  Everywhere else 1 ulp is the binding condition.
      The stand-in's linear accumulates like a matrix pipe (`_mm`); see GAINS for the input scales SHARE needs.
  a, lse of the flash forward, dQ / dK / dV of its backward: the attention kernel's own bars (FWD_BARS, LSE_BAR, BWD_BARS); an `a` written
      in T adds u / sqrt 3 of T's unit roundoff u in quadrature (`a_bar`).

Mutants (each one defect in the stand-in; tests/test_mixed_audit_cpu.py): all four break the audit by >= 5 bars in both precisions.  What a
plain two-block float64 step shows of the same defect, per parameter rel-L2, against the old bars (fp16 1e-2 / bf16 1.3e-1):
  wgrad_loses_the_last_token_row        fc1.weight 6.0e-2 (one of 84 rows: fails fp16's bar at this size, passes bf16's); audit 8,000 bars
  residual_kept_in_16_bits              5.3e-4 fp16 / 4.5e-3 bf16: passes both;   audit 44 / 444 bars (x1 itself)
  bias_gradient_from_the_rounded_image  1.9e-4 fp16 / 1.7e-3 bf16: passes both;   audit 29 / 274 bars (proj.bias)
  dq_scale_dropped                      caught by the BWD_BARS check: dQ off by 7.0 (rel-L2) against 8.5e-4 / 1.1e-2
"""
import contextlib
import functools
import math
import types
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

import train_parity
from mst import synth

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
SOURCE = train_parity.SOURCE
NOISE = 1e-6        # fp32-valued stand-in against float64: measured worst over RUNS x both precisions 9.7e-7 (b0.dY.mlp.fc1 of mlp_m63)
BAR = 1e-5          # 10 x NOISE
SHARE = 1e-3
# tests/test_attn_train_gpu.py::test_forward_and_lse_against_fp64: rel-L2 of O, max |d LSE|
FWD_BARS = {"fp16": 1.8e-4, "bf16": 1.4e-3}
LSE_BAR = 8.5e-6
UNIT_ROUNDOFF = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}          # |r(x) - x| <= u |x|

# Measured on the MI355X (fp16 / bf16, fp32 storage and 16-bit storage alike unless two values are given as fp32 | 16bit):
#   case      fp32-valued worst      T tensors: not bit-equal (worst), worst ulp     a rel-L2             dQ / dK / dV rel-L2 (worst)
#   mlp_m84   1.3e-6 / 1.1e-6        7.1e-4 / 1.3e-4, 4 / 3 ulp, none off            8.2e-5 | 2.3e-4 / 6.4e-4 | 1.8e-3   5.4e-4 / 4.9e-3
#   mlp_m63   1.4e-6 / 1.1e-6        7.4e-4 / 1.2e-4, 4 / 1 ulp, none off            8.5e-5 | 2.2e-4 / 6.6e-4 | 1.8e-3   5.1e-4 / 4.8e-3
#   ls_reg    1.0e-6 / 9.2e-7        7.7e-4 / 1.6e-4, 3 / 3 ulp, none off            8.1e-5 | 2.2e-4 / 6.3e-4 | 1.8e-3   4.3e-4 / 4.4e-3
#   swiglu    9.4e-7 / 1.2e-6        7.0e-4 / 1.3e-4, 4 / 3 ulp, none off            8.0e-5 | 2.2e-4 / 6.1e-4 | 1.8e-3   4.3e-4 / 5.5e-3
#   mlp_m84, stored attention: 1.2e-6 / 1.3e-6 (no tensor in T).  LSE within 1.6e-6 everywhere.
# Bars: 1e-5; 1e-3 and 1 ulp-or-BAR; a 1.8e-4 | 3.3e-4 / 1.4e-3 | 2.7e-3; dqkv 8.5e-4 / 1.1e-2; LSE 8.5e-6.
CASES = {  # name -> embed dim, heads, depth, slices, H, W, stored position grid (img_size), register tokens, LayerScale, FFN
    "mlp_m84": dict(E=384, heads=6, depth=2, n=4, H=70, W=56, img=224, reg=0, ls=False, ffn="mlp"),      # N = 21, M = 84: not a multiple of 64; two blocks: the xn hand-off, nxt is None
    "mlp_m63": dict(E=384, heads=6, depth=2, n=3, H=70, W=56, img=224, reg=0, ls=False, ffn="mlp"),      # M = 63 < 64: every lin_bwd on the fp32 fallback behind a 16-bit forward
    "ls_reg": dict(E=384, heads=6, depth=1, n=4, H=56, W=56, img=56, reg=4, ls=True, ffn="mlp"),         # LayerScale, 4 registers: colsum(b=16-bit br), axpby_cols(g=), d register_tokens
    "swiglu": dict(E=384, heads=6, depth=1, n=4, H=70, W=56, img=224, reg=0, ls=False, ffn="swiglufused"),   # x12 / h saved, swiglu_bwd between two lin_bwd calls
    "swiglu_e128": dict(E=128, heads=2, depth=1, n=4, H=70, W=56, img=224, reg=0, ls=False, ffn="swiglufused"),
}
# swiglu_e128 (w12 with N = 688, w3 with K = 344: both off the 16-bit route inside one block) is not run: the 16-bit FORWARD refuses the
# width -- "gemm16: N=688 must be a multiple of 128" -- before any backward route is chosen.  tests/test_mixed_audit_gpu.py asserts that.
REFUSED = "swiglu_e128"
MODES = [("fp32", "flash"), ("16bit", "flash")]                   # (train_storage, train_attention) of every case
STORED_CASE = ("mlp_m84", "fp32", "stored")                       # fp32 qkv and P: another rounding set
RUNS = [(c, s, a) for c in CASES if c != REFUSED for s, a in MODES] + [STORED_CASE]
STATE_SEED, VOLUME_SEED, GRAD_SEED = 57, 157, 257


class Cfg(NamedTuple):
    T: Optional[torch.dtype]                                      # None: no rounding anywhere (the plain float64 step)
    storage16: bool
    flash: bool
    n: int
    N: int
    heads: int
    E: int


def tokens_per_slice(case):
    c = CASES[case]
    return 1 + c["reg"] + (c["H"] // 14) * (c["W"] // 14)


def cfg_of(case, prec, storage, attn):
    c = CASES[case]
    return Cfg(DT[prec] if prec else None, storage == "16bit", attn == "flash", c["n"], tokens_per_slice(case), c["heads"], c["E"])


# Scales of the blocks' nn.Linear (weight gain, bias gain) on top of synth_state_dict's, chosen so that the 16-bit condition can be met at
# all.  With its own scales an output is a sum of K random-sign products, and an fp32 accumulator leaves sqrt(K) * 1e-4 of the fp16
# outputs on the other side of a rounding boundary from the float64 value: measured on the MI355X 7.0e-4 of qkv16 (K = 384), 1.5e-3 of
# br2 (K = 1536), 9.3e-4 of hact (the fp32 GELU's 1 + erf below zero) not bit-equal -- next to SHARE or above it, whatever the kernel.  A bias
# larger than the product keeps the outputs off zero, where an ulp is smallest; every product, rounding and route is still run.
#   fc1 / w12: bias std 0.5 beside a product of 0.3 -- it stays inside the MLP.
#   proj / fc2 / w3: the product shrinks under synth's own bias (std 0.05).  A large bias here is one vector added to every token of the
#       residual stream: the next block's v rows share an offset, dS = P (dP - D) becomes a small difference of large terms and the
#       attention kernel's 16-bit dS shows in dQ (measured 9.3e-4 .. 1.2e-3 in fp16 against BWD_BARS' 8.5e-4).
#   qkv: untouched, so that q, k, v stay where BWD_BARS were measured (scores with a spread of 2.5): 3.7e-4 .. 5.4e-4.
GAINS = {"attn.proj": (0.02, 1.0), "mlp.fc2": (0.02, 1.0), "mlp.w3": (0.02, 1.0), "mlp.fc1": (0.25, 10.0), "mlp.w12": (0.25, 10.0)}
_SHRINK = {384: 128, 1152: 384, 2048: 688, 1024: 344}             # ViT-S shapes -> E = 128, 2 heads, SwiGLU hidden 344


@functools.lru_cache(maxsize=None)
def encoder_state(case):
    """{'encoder.<key>': fp32 tensor} of the case's `_ViT` (hub layout: blocks.<i>).  E = 384: synth_state_dict's own tensors; E = 128:
    their leading sub-blocks, matrices times sqrt(3) to keep the fan-in scaling.  Memoised: leave the tensors unchanged."""
    c = CASES[case]
    sd = synth.synth_state_dict("s", STATE_SEED, img_size=c["img"], layerscale=c["ls"], chunked=False, num_register_tokens=c["reg"],
                                ffn_layer=c["ffn"], depth=c["depth"])
    sd = {k: v for k, v in sd.items() if k.startswith("encoder.")}
    for k in sd:
        lin, _, what = k.rpartition(".")
        for name, (wg, bg) in GAINS.items():
            if lin.endswith(name):
                sd[k] = sd[k] * (wg if what == "weight" else bg)
    if c["E"] == 384:
        return sd
    assert c["E"] == 128
    out = {}
    for k, v in sd.items():
        w = v[tuple(slice(0, _SHRINK.get(d, d)) for d in v.shape)].clone()
        out[k] = w * math.sqrt(3.0) if (w.dim() == 2 and k.endswith(".weight")) else w
    return out


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(slices [n, H, W], d embeddings [n, E], the dense term added to the gradient entering the last block [n * N, E]), fp32."""
    c = CASES[case]
    vol = synth.synth_volume((1, 1, c["n"], c["H"], c["W"]), VOLUME_SEED)[0, 0].contiguous()
    demb = torch.from_numpy(synth.hash_normal((c["n"], c["E"]), GRAD_SEED, 1))
    dense = torch.from_numpy(synth.hash_normal((c["n"] * tokens_per_slice(case), c["E"]), GRAD_SEED, 2)) * 0.25
    return vol, demb, dense


# ---------------------------------------------------------------------------------------------------------------------------------
# the segment arithmetic, generic in the working type dt (float64: the reference; float32: the stand-in)
# ---------------------------------------------------------------------------------------------------------------------------------
def rnd(x, T):
    """x rounded to T, in x's own type (T None: x).  Values only: call it on detached tensors."""
    return x if T is None else x.to(T).to(x.dtype)


KSTEP = 16


def _mm(a, b, pipe):
    """a [M, K] . b [K, N].  float64, or an fp32 product of the stand-in's fallback route: the plain product.  A product of 16-bit operands
    in float32 (`pipe`; the stand-in): as a matrix pipe accumulates -- K-steps of KSTEP exact products summed and rounded to fp32 once,
    the steps added in fp32 in ascending order.  (A plain fp32 dot product, one rounding per product, leaves 1.7e-3 of the fp16 outputs at
    K = 384 not bit-equal to the rounded float64 value, the MI355X 7e-4, this form 5.5e-4.)"""
    if a.dtype == torch.float64 or not pipe:
        return a @ b
    acc = torch.zeros(a.shape[0], b.shape[1], dtype=torch.float32)
    for k in range(0, a.shape[1], KSTEP):
        acc = acc + (a[:, k:k + KSTEP].double() @ b[k:k + KSTEP].double()).float()
    return acc


def gelu(x):
    """GELU (erf) as 0.5 x erfc(-x / sqrt 2): no cancellation for x < 0 in either type."""
    return 0.5 * x * torch.special.erfc(x * (-1.0 / math.sqrt(2.0)))


class _Lin(torch.autograd.Function):
    """nn.Linear as the 16-bit step runs it.  Forward r(x) . r(W)^T + b.  Backward on the 16-bit route (`route16`): dX = r(dY) . r(W),
    dW = r(dY)^T . r(x), db = sum of the unrounded dY; on the fp32 fallback nothing is rounded (x is the saved tensor as it is).
    `mut`: the defects of MUTANTS that live in a linear's backward."""

    @staticmethod
    def forward(ctx, x, W, b, T, route16, mut, gtap):
        ctx.save_for_backward(x, W)
        ctx.meta = (T if route16 else None, mut, gtap)
        return _mm(rnd(x, T), rnd(W, T).t(), T is not None) + b

    @staticmethod
    def backward(ctx, dY):
        x, W = ctx.saved_tensors
        Tb, mut, gtap = ctx.meta
        dY = gtap(dY)                                             # the gradient `lin_bwd` was called with, as recorded
        dYr = rnd(dY, Tb)
        dX = _mm(dYr, rnd(W, Tb), Tb is not None)
        xs = rnd(x, Tb)
        dW = _mm(dYr[:-1].t(), xs[:-1], Tb is not None) if mut.get("drop_last_row") else _mm(dYr.t(), xs, Tb is not None)
        db = rnd(dY, mut["db_T"]).sum(0) if "db_T" in mut else dY.sum(0)
        return dX, dW, db, None, None, None, None


def _heads(qkv, c: Cfg):
    x = qkv.view(c.n, c.N, 3, c.heads, c.E // c.heads).permute(2, 0, 3, 1, 4)                 # [3, n, heads, N, 64]
    return x[0], x[1], x[2]


def attention_fwd(qkv, c: Cfg):
    """(O [n*N, E], LSE [n, heads, N]) of softmax(q k^T) v on packed rows in qkv's type.  Nothing is rounded inside: the attention core is
    not modelled, in the stand-in no more than in the reference (the kernel's 16-bit probabilities are what FWD_BARS grant)."""
    q, k, v = _heads(qkv, c)
    s = q @ k.transpose(-1, -2)
    out = torch.softmax(s, dim=-1) @ v
    return out.transpose(1, 2).reshape(c.n * c.N, c.E), torch.logsumexp(s, dim=-1)


def attention_bwd(qkv, dout, c: Cfg, dq_scale):
    """Autograd of O = softmax(q k^T) v in qkv's type: dqkv [n*N, 3E] with dQ times dq_scale (tests/test_attn_train_gpu.py::_ref_bwd)."""
    q, k, v = (t.detach().clone().requires_grad_(True) for t in _heads(qkv, c))
    o = (torch.softmax(q @ k.transpose(-1, -2), dim=-1) @ v).transpose(1, 2).reshape(c.n * c.N, c.E)
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), dout.to(qkv.dtype))
    return torch.stack([gq * dq_scale, gk, gv]).permute(1, 3, 0, 2, 4).reshape(c.n * c.N, 3 * c.E)


def block_graph(p, s, dys, c: Cfg, dt, mut, create):
    """The autograd graph of one block in dt from the saved x0.  p: the block's parameters in dt ({'norm1.weight': ...}, requires_grad);
    s: the block's record.  create False (the audit): every stage is computed from the SAVED tensors before it, its own value goes to
    out[name] and downstream sees the saved value.  create True (the stand-in): the stage's value is stored into s as the step stores
    it -- rounded to T where the step writes T -- and downstream reads that.  dys: {linear: the dY its `lin_bwd` was called with}, treated
    in the backward as s is in the forward: the reference's own dY goes to out_g, the linear's three products read the recorded one, so that
    r(dY) is the same image on both sides and no rounding of a gradient can fall differently."""
    T, E = c.T, c.E
    out, out_g = {}, {}

    def gtap(name):
        def f(dY):
            out_g[name] = dY
            if create:
                dys[name] = dY.to(torch.float32) if T is not None else dY
            return dys[name].to(dt)
        return f

    def tap(name, ref):
        out[name] = ref.detach()
        if create:
            v = ref.detach()
            if name == "x1" and "x1_T" in mut:
                v = rnd(v, mut["x1_T"])
            in_T = T is not None and (name == "qkv16" or (c.storage16 and name not in ("x1", "lse")))
            s[name] = v.to(T) if in_T else (v.to(torch.float32) if T is not None else v)
        return ref + (s[name].to(dt) - ref).detach()

    def ln(x, name):
        return F.layer_norm(x, (E,), p[name + ".weight"], p[name + ".bias"], 1e-6)

    def lin(name, x):
        W = p[name + ".weight"]
        route16 = T is not None and W.shape[0] % 128 == 0 and W.shape[1] % 128 == 0 and x.shape[0] >= 64
        return _Lin.apply(x, W, p[name + ".bias"], T, route16, mut.get(name, {}), gtap(name))

    x0 = s["x0"].to(dt).clone().requires_grad_()
    xn1 = tap("xn1", ln(x0, "norm1"))
    pre = lin("attn.qkv", xn1)                                    # the projection before its epilogue's factor: dqkv is its gradient
    cs = torch.ones(3 * E, dtype=dt)
    cs[:E] = 0.125
    a_leaf = None
    if c.flash:
        tap("qkv16", pre * cs)
        a_ref, lse_ref = attention_fwd(s["qkv16"].to(dt), c)
        tap("lse", lse_ref)
        a_leaf = tap("a", a_ref).detach().clone().requires_grad_()   # the chain is cut here: `a` is the saved value
        a = a_leaf
    else:
        q, k, v = _heads(tap("qkv", pre * cs), c)
        P = tap("P", torch.softmax(q @ k.transpose(-1, -2), dim=-1))
        a = tap("a", (P @ v).transpose(1, 2).reshape(c.n * c.N, E))
    br1 = tap("br1", lin("attn.proj", a))
    x1 = tap("x1", x0 + (br1 * p["ls1.gamma"] if "ls1.gamma" in p else br1))
    xn2 = tap("xn2", ln(x1, "norm2"))
    if "mlp.w12.weight" in p:
        x12 = tap("x12", lin("mlp.w12", xn2))
        H = x12.shape[1] // 2
        br2 = tap("br2", lin("mlp.w3", tap("h", F.silu(x12[:, :H]) * x12[:, H:])))
    else:
        hpre = tap("hpre", lin("mlp.fc1", xn2))
        br2 = tap("br2", lin("mlp.fc2", tap("hact", gelu(hpre))))
    x2 = x1 + (br2 * p["ls2.gamma"] if "ls2.gamma" in p else br2)
    out["x2"] = x2.detach()
    return dict(x0=x0, pre=pre, a_leaf=a_leaf, x2=x2, out=out, out_g=out_g)


def block_backward(g, s, c: Cfg, dt, dx_in, dqkv=None, dq_scale=0.125):
    """d x2 = dx_in through the graph: parameter gradients into the parameters' .grad; returns (dx0, da or None, the dqkv used or None).
    dqkv None with a cut graph: the attention core's gradient is this module's own (the stand-in); given: the recorded one (the audit)."""
    g["x2"].backward(dx_in.to(dt), retain_graph=True)
    da = None
    if g["a_leaf"] is not None:
        da = g["a_leaf"].grad
        if dqkv is None:
            dqkv = attention_bwd(s["qkv16"].to(dt), da, c, dq_scale)
        g["pre"].backward(dqkv.to(dt))
    return g["x0"].grad, da, dqkv


def _block_params(P, i):
    pre = f"encoder.blocks.{i}."
    return {k[len(pre):]: v for k, v in P.items() if k.startswith(pre)}


def _tokens(P, vol):
    from oracle import mst_oracle as O
    n = vol.shape[0]
    x = O.prepare_tokens(P, vol)
    return x.reshape(n * x.shape[1], x.shape[2])


def _params(case, dt):
    return {k: v.to(dt).clone().requires_grad_() for k, v in encoder_state(case).items() if k != "encoder.mask_token"}


def _cls_norm(P, xL, c: Cfg):
    return F.layer_norm(xL.view(c.n, c.N, c.E)[:, 0], (c.E,), P["encoder.norm.weight"], P["encoder.norm.bias"], 1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
# the CPU stand-in of the HIP step and its mutants
# ---------------------------------------------------------------------------------------------------------------------------------
_ACTIVE = {}


@contextlib.contextmanager
def _mutant(**kw):
    _ACTIVE.update(kw)
    try:
        yield
    finally:
        for k in kw:
            _ACTIVE.pop(k)


def wgrad_loses_the_last_token_row():
    """fc1's weight-gradient product ignores the last token row: a ragged tail lost in a padded operand image."""
    return _mutant(**{"mlp.fc1": {"drop_last_row": True}})


def residual_kept_in_16_bits(T):
    """The residual stream x1 is stored in T instead of fp32."""
    return _mutant(x1_T=T)


def bias_gradient_from_the_rounded_image(T):
    """proj's bias gradient is summed from r(dY) instead of the fp32 dY."""
    return _mutant(**{"attn.proj": {"db_T": T}})


def dq_scale_dropped():
    """attention_train_bwd called without dq_scale = 0.125."""
    return _mutant(dq_scale=1.0)


MUTANTS = {  # name -> (context manager taking T, (case, storage, attention) it is measured on)
    "wgrad_loses_the_last_token_row": (lambda T: wgrad_loses_the_last_token_row(), ("mlp_m84", "fp32", "flash")),
    "residual_kept_in_16_bits": (residual_kept_in_16_bits, ("mlp_m84", "16bit", "flash")),
    "bias_gradient_from_the_rounded_image": (bias_gradient_from_the_rounded_image, ("mlp_m84", "16bit", "flash")),
    "dq_scale_dropped": (lambda T: dq_scale_dropped(), ("mlp_m84", "16bit", "flash")),
}


def standin_step(case, prec, storage, attn, dt=torch.float32):
    """The step's record from torch on the CPU: the segments chained in dt with the step's roundings (prec None: none at all, dt float64 --
    the plain step the old whole-step bars are read against), under whatever mutant is active.  The layout of `hip_step`'s record."""
    c = cfg_of(case, prec, storage, attn)
    mut = dict(_ACTIVE)
    vol, demb, dense = inputs(case)
    P = _params(case, dt)
    v = vol.to(dt).clone().requires_grad_()
    x_tok = _tokens(P, v)
    x, blocks, graphs, dys = x_tok.detach(), [], [], []
    for i in range(CASES[case]["depth"]):
        s = {"x0": x.to(torch.float32) if c.T is not None else x}
        dys.append({})
        g = block_graph(_block_params(P, i), s, dys[-1], c, dt, mut, create=True)
        blocks.append(s)
        graphs.append(g)
        x = g["out"]["x2"]
    xL = (x.to(torch.float32) if c.T is not None else x)
    xLg = xL.to(dt).clone().requires_grad_()
    emb = _cls_norm(P, xLg, c)
    emb.backward(demb.to(dt))
    dx = xLg.grad + dense.to(dt)
    rec = dict(blocks=blocks, dY=dys, xL=xL, emb=emb.detach(), dx_in=[None] * len(blocks), dx0=[None] * len(blocks), attn=[None] * len(blocks))
    for i in reversed(range(len(blocks))):
        rec["dx_in"][i] = dx.to(torch.float32) if c.T is not None else dx
        dx, da, dqkv = block_backward(graphs[i], blocks[i], c, dt, rec["dx_in"][i], None, mut.get("dq_scale", 0.125))
        dx = dx.to(torch.float32).to(dt) if c.T is not None else dx
        rec["dx0"][i] = dx.to(torch.float32) if c.T is not None else dx
        if da is not None:
            rec["attn"][i] = dict(da=da.float(), dqkv=dqkv.float())
    x_tok.backward(dx)
    rec["grads"] = {k: p.grad for k, p in P.items()}
    rec["grads"][SOURCE] = v.grad
    if c.T is not None:
        rec["grads"] = {k: g.float() for k, g in rec["grads"].items()}
    return rec


# ---------------------------------------------------------------------------------------------------------------------------------
# the HIP step, recorded
# ---------------------------------------------------------------------------------------------------------------------------------
def build_encoder(case):
    from mst.models.dino import _ViT
    c = CASES[case]
    enc = _ViT(c["E"], c["depth"], c["heads"], img_size=c["img"], num_register_tokens=c["reg"], layerscale=1.0 if c["ls"] else None,
               chunked=False, ffn_layer=c["ffn"])
    enc.load_state_dict({k[len("encoder."):]: v for k, v in encoder_state(case).items()}, strict=True)
    return enc.cuda()


def hip_step(case, prec, storage, attn, monkeypatch):
    """`_encoder_fwd` and `_encoder_bwd` (need_src) of mst/train.py on the case's encoder in the given mode, recorded: the saved state, the
    gradient entering and leaving every block (clones behind every mst_layernorm_bwd; the first one, the final norm's, gets the dense
    term added in place), the arguments and the result of every attention_train_bwd, every gradient.  Also asserts the hand-off rules of
    the forward by identity.  Returns the record on the CPU."""
    from mst import hip, train
    from mst.train_mode import TrainMode
    c = CASES[case]
    vol, demb, dense = (t.cuda() for t in inputs(case))
    enc = build_encoder(case)
    mode = TrainMode(DT[prec], attn == "flash", storage == "16bit", 0)
    hand, dxs, att, dys = [], [], [], {}
    names = {id(mod): k for k, mod in enc.named_modules()}
    fwd_name = "_block_fwd_16" if mode.storage16 else "_block_fwd"
    fwd, ln_bwd, attn_bwd, lin_bwd = getattr(train, fwd_name), hip.layernorm_bwd, hip.attention_train_bwd, train._Grads.lin_bwd

    def rec_fwd(*a):
        r = fwd(*a)
        hand.append((a[3], r[1], r[2]))                            # the xn it was given, x2, the xn it hands on
        return r

    def rec_ln_bwd(*a):
        ln_bwd(*a)
        if not dxs:
            a[7].add_(dense)
        dxs.append(a[7].clone())

    def rec_lin_bwd(self, dY, X, lin, *a, **kw):
        assert names[id(lin)] not in dys
        dys[names[id(lin)]] = dY.clone()
        return lin_bwd(self, dY, X, lin, *a, **kw)

    def rec_attn_bwd(qkv16, a, da, lse, *rest, **kw):
        assert kw == {"dq_scale": 0.125} or (len(rest) == 4 and rest[3] == 0.125), (rest, kw)
        r = attn_bwd(qkv16, a, da, lse, *rest, **kw)
        att.append(dict(qkv16=qkv16.clone(), a=a.clone(), da=da.clone(), lse=lse.clone(), dqkv=r.clone()))
        return r

    H, W = c["H"], c["W"]
    interp = not ((H // 14) * (W // 14) == enc.pos_embed.shape[1] - 1 and H == W)
    sv = {"interp": interp, "H": H, "W": W, "mp": mode.mp, "vol": vol}
    model = types.SimpleNamespace(encoder=enc)
    with monkeypatch.context() as m, torch.no_grad():
        m.setattr(train, fwd_name, rec_fwd)
        m.setattr(train.hip, "layernorm_bwd", rec_ln_bwd)
        m.setattr(train.hip, "attention_train_bwd", rec_attn_bwd)
        m.setattr(train._Grads, "lin_bwd", rec_lin_bwd)
        emb = train._encoder_fwd(model, sv, mode, vol, c["n"], H, W)
        G = train._Grads()
        dvol = train._encoder_bwd(G, model, sv, demb, c["n"], True)
        torch.cuda.synchronize()
    depth, blocks = c["depth"], sv["blocks"]
    assert len(hand) == depth and len(dxs) == 1 + 2 * depth and len(att) == (depth if mode.flash else 0)
    for i, s in enumerate(blocks):
        nxt_x0 = blocks[i + 1]["x0"] if i + 1 < depth else sv["xL"]
        assert nxt_x0.data_ptr() == hand[i][1].data_ptr(), "x0 of the next block is not this block's x2"
        if not mode.storage16:
            assert hand[i][2] is None
            continue
        assert s["xn1"].data_ptr() == hand[i][0].data_ptr()
        if i + 1 < depth:                                          # the next block's xn1 IS what this block's closing LayerNorm wrote
            assert hand[i][2] is not None and blocks[i + 1]["xn1"].data_ptr() == hand[i][2].data_ptr()
        else:
            assert hand[i][2] is None, "a LayerNorm behind the last block"
    for i, s in enumerate(blocks):                                 # the record the kernel was given is the saved one
        if mode.flash:
            a = att[depth - 1 - i]
            assert torch.equal(a["qkv16"], s["qkv16"]) and torch.equal(a["a"], s["a"]) and torch.equal(a["lse"], s["lse"])
    cpu = lambda t: t.detach().cpu()
    rec = dict(blocks=[{k: cpu(v) for k, v in s.items() if torch.is_tensor(v)} for s in blocks], xL=cpu(sv["xL"]), emb=cpu(emb),
               dY=[{k[len(f"blocks.{i}."):]: cpu(v) for k, v in dys.items() if k.startswith(f"blocks.{i}.")} for i in range(depth)],
               dx_in=[cpu(dxs[2 * (depth - 1 - i)]) for i in range(depth)], dx0=[cpu(dxs[2 * (depth - 1 - i) + 2]) for i in range(depth)],
               attn=[dict(da=cpu(att[depth - 1 - i]["da"]), dqkv=cpu(att[depth - 1 - i]["dqkv"])) if mode.flash else None
                     for i in range(depth)])
    rec["grads"] = {"encoder." + k: cpu(G.by_param[id(p)]) for k, p in enc.named_parameters() if id(p) in G.by_param}
    rec["grads"][SOURCE] = cpu(dvol)
    return rec


# ---------------------------------------------------------------------------------------------------------------------------------
# the audit
# ---------------------------------------------------------------------------------------------------------------------------------
def _ordinal(t):
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulp_compare(got, ref64):
    """(largest distance in ulps of got's type between got and r(ref), share of elements that are not bit-equal, elements further than
    1 ulp from r(ref) AND further than BAR * max |ref| from ref: the ones that break the condition of the module docstring)."""
    d = (_ordinal(got) - _ordinal(ref64.to(got.dtype))).abs()
    far = (got.double() - ref64).abs() > BAR * float(ref64.abs().max())
    return int(d.max()), float((d != 0).double().mean()), int(((d > 1) & far).sum())


def _scaled(got, ref):
    return float((got.double() - ref.double()).abs().max()) / float(ref.double().abs().max())


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def audit(rec, case, prec, storage, attn):
    """The record against float64, stage by stage.  Returns
      f32:   {name: max |d| / max |ref|}      fp32-valued tensors: saved ones (b<i>.<name>), gradients (by parameter), dx0, da, d volume
      t16:   {name: (max ulp, share not bit-equal)}   tensors saved in T
      attn:  {name: value}                     a (rel-L2) and lse (max abs) of the flash forward, dQ / dK / dV (rel-L2) of its backward."""
    c = cfg_of(case, prec, storage, attn)
    dt = torch.float64
    vol, demb, dense = inputs(case)
    res = dict(f32={}, t16={}, attn={})

    def compare(tag, got, ref):
        if got.dtype in (torch.float16, torch.bfloat16):
            assert got.dtype == c.T, (tag, got.dtype)
            res["t16"][tag] = ulp_compare(got, ref)
        else:
            assert got.dtype == torch.float32, (tag, got.dtype)
            res["f32"][tag] = _scaled(got, ref)

    P = _params(case, dt)
    depth = CASES[case]["depth"]
    # token stage and final norm: fp32 ops, exact in float64
    v = vol.to(dt).clone().requires_grad_()
    x_tok = _tokens(P, v)
    compare("tokens", rec["blocks"][0]["x0"], x_tok.detach())
    xL = rec["xL"].to(dt).clone().requires_grad_()
    emb = _cls_norm(P, xL, c)
    compare("emb", rec["emb"], emb.detach())
    emb.backward(demb.to(dt))
    compare("dx_in", rec["dx_in"][-1], xL.grad + dense.to(dt))
    for i in reversed(range(depth)):
        s = rec["blocks"][i]
        for k, t in s.items():                                     # the storage rule of the mode
            want = c.T if (k == "qkv16" or (c.storage16 and k not in ("x0", "x1", "lse"))) else torch.float32
            assert t.dtype == want, (k, t.dtype, want)
        g = block_graph(_block_params(P, i), s, rec["dY"][i], c, dt, {}, create=False)
        for k, ref in g["out"].items():
            got = (rec["blocks"][i + 1]["x0"] if i + 1 < depth else rec["xL"]) if k == "x2" else s[k]
            if c.flash and k == "a":
                res["attn"][f"b{i}.a"] = _rel(got, ref)
            elif k == "lse":
                res["attn"][f"b{i}.lse"] = float((got.double() - ref).abs().max())
            else:
                compare(f"b{i}.{k}", got, ref)
        ar = rec["attn"][i]
        dx0, da, _ = block_backward(g, s, c, dt, rec["dx_in"][i], ar["dqkv"] if ar else None)
        compare(f"b{i}.dx0", rec["dx0"][i], dx0)
        assert set(g["out_g"]) == set(rec["dY"][i]), sorted(set(g["out_g"]) ^ set(rec["dY"][i]))
        for k, ref in g["out_g"].items():
            compare(f"b{i}.dY.{k}", rec["dY"][i][k], ref)
        if ar:
            compare(f"b{i}.da", ar["da"], da)
            ref = attention_bwd(s["qkv16"].to(dt), ar["da"].to(dt), c, 0.125).view(-1, 3, c.E)
            got = ar["dqkv"].view(-1, 3, c.E)
            for j, nm in enumerate(("dQ", "dK", "dV")):
                res["attn"][f"b{i}.{nm}"] = _rel(got[:, j], ref[:, j])
    x_tok.backward(rec["dx0"][0].to(dt))
    ref = {k: p.grad for k, p in P.items()}
    ref[SOURCE] = v.grad
    for k, e in train_parity.scaled_errors(rec["grads"], ref).items():
        assert rec["grads"][k].dtype == torch.float32, k
        res["f32"][k] = e
    return res


def a_bar(prec, storage):
    """rel-L2 bar of the flash forward's output: the kernel's own; where the epilogue rounds to T, in quadrature with u / sqrt 3 -- the
    root mean square of a relative rounding error spread evenly over [-u, u], which round-to-nearest stays below in every binade."""
    return math.hypot(FWD_BARS[prec], UNIT_ROUNDOFF[prec] / math.sqrt(3.0)) if storage == "16bit" else FWD_BARS[prec]


def failures(res, prec, storage, bar):
    """The entries of an audit that break their bar, as strings (empty: the record passes)."""
    from test_attn_train_gpu import BWD_BARS
    bad = [f"{k} {e:.3e} > {bar:g}" for k, e in res["f32"].items() if not e <= bar]
    bad += [f"{k} {n} elements off (worst {u} ulp), {sh:.2e} not bit-equal" for k, (u, sh, n) in res["t16"].items() if n or sh > SHARE]
    for k, e in res["attn"].items():
        lim = a_bar(prec, storage) if k.endswith(".a") else LSE_BAR if k.endswith(".lse") else BWD_BARS[prec]
        if not e < lim:
            bad.append(f"{k} {e:.3e} >= {lim:.3g}")
    return bad


def worst(res):
    """One line: the worst entry of each kind."""
    f = max(res["f32"], key=res["f32"].get)
    line = f"f32 {res['f32'][f]:.2e} ({f})"
    if res["t16"]:
        u = max(res["t16"], key=lambda k: res["t16"][k])
        sh = max(res["t16"], key=lambda k: res["t16"][k][1])
        line += f", T {res['t16'][u][0]} ulp ({u}), {sum(v[2] for v in res['t16'].values())} off, not bit-equal {res['t16'][sh][1]:.2e} ({sh})"
    if res["attn"]:
        line += ", " + " ".join(f"{k} {e:.1e}" for k, e in res["attn"].items())
    return line
