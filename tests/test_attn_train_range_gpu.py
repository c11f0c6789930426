"""Dynamic range, per-head accuracy and tile seams of the training attention (csrc/k_attn16_train.hip): forward with LSE, preprocess, key
pass and query pass against fp64 on the same rounded operands (tests/attn_train_ref.py), per (sequence, head) and per tensor.

  A  tile seams: N around 32, 64, 96, 128, 160          E  score structure: offsets, a dominant key, identical keys, all very negative
  B  power-of-two homogeneity of the backward in dO      F  dO in one query row only (row 0, row N-1)
  C  dO magnitudes that differ per (sequence, head)      G  fp16 headroom of dS
  D  bottom and top of the range of dO

Bars: 4 x the worst per-head error of the fp32 emulation of the kernels' rounding points on the same inputs (attn_train_ref.EMU, kept
current by test_attn_train_range_cpu.py); the factor covers the MFMA accumulation order, v_exp_f32 against exp and the log2 e / ln 2 round
trip.  The LSE bar of the offset inputs is attn_train_ref.lse_bound, derived from fp32's unit roundoff.  Bit-equality takes no bar.

D, the tiny heads: a head whose max |dO| is 2^-124, and one at 1e-40 (a denormal), are held to the same kind of bar as every other head
-- their gradients are fp32 denormals, which the emulation rounds like the kernel does -- and are not allowed to be zero.  Before the
exponent of the scale was bounded, every gradient of both heads was non-finite on the MI355X (24,960 of the 49,920 elements of dqkv, in
both types: c = 2^129 and 2^138 are inf, so dO c and D are inf and dP - D is NaN); the two unit-scale heads were right.

Set MST_ATTN_RANGE_LOG to a file name to get one JSON line per case with the measured errors beside the emulation's
(profiles/attn_train_range.jsonl is the MI355X's record, worst per family)."""

import json
import os

import pytest
import torch

import attn_train_ref as R
from mst import hip

pytestmark = pytest.mark.gpu

PRECS = list(R.DT)
DQ = 0.125


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _cuda(c):
    return c._replace(qkv=c.qkv.cuda(), dout=c.dout.cuda())


def _log(family, prec, case, measured):
    emu = R.EMU[family][prec]
    print(f"{family} {prec} {case}: " + ", ".join(f"{k} {v:.3e} (emulation {emu[k]:.3e})" if k in emu else f"{k} {v:.3e}"
                                                  for k, v in measured.items()))
    path = os.environ.get("MST_ATTN_RANGE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"family": family, "prec": prec, "case": case, "measured": measured,
                                "emulation": {k: emu[k] for k in measured if k in emu}}) + "\n")


def _forward(family, prec, c, lse_bar=None):
    """out, lse of the kernel, O per head within the bar, LSE within its bar (the family's, or an elementwise lse_bar)."""
    out, lse = hip.attention_train_fwd(c.qkv, c.n, c.N, c.heads)
    O, L = R.ref_fwd(c.qkv, c.n, c.heads, c.N)
    e_o, where = R.worst(R.head_errors(out, O, c.n, c.N, c.heads)[0])
    d = (lse.double() - L).abs()
    e_l = float(d.max()) if bool(torch.isfinite(d).all()) else float("inf")
    got = {"O": e_o, "LSE": e_l}
    if lse_bar is not None:
        got["LSE_over_bound"] = float((d / lse_bar).max())
    _log(family, prec, c.name, got)
    assert e_o <= R.bar(family, prec, "O"), (e_o, where)
    if lse_bar is None:
        assert e_l <= R.bar(family, prec, "LSE"), e_l
    else:
        assert bool((d <= lse_bar).all()), got
    return out, lse


def _backward(family, prec, c, out, lse, tiny=None):
    """dqkv of the kernel, every (sequence, head) of dQ, dK, dV within the bar; heads whose reference is exactly zero must be zero.
    tiny: {(sequence, head): suffix} of heads with bars of their own (family D)."""
    dqkv = hip.attention_train_bwd(c.qkv, out, c.dout, lse, c.n, c.N, c.heads, dq_scale=DQ)
    ref = R.ref_bwd(c.qkv, c.dout, c.n, c.heads, c.N, DQ)
    e = R.head_errors(dqkv, ref, c.n, c.N, c.heads, R.WHOLE.get(family, ()))
    zero = ref.view(c.n, c.N, 3, c.heads, 64).abs().amax((1, 4)).permute(1, 0, 2) == 0
    assert bool((e[zero] == 0).all()), e
    e = torch.where(zero, torch.zeros_like(e), e)
    got = {}
    for (s, h), name in (tiny or {}).items():
        for i, t in enumerate(R.NAMES):
            got[f"{t}_{name}"] = float(e[i, s, h])
        e[:, s, h] = 0
    where = {}
    for i, t in enumerate(R.NAMES):
        got[t], where[t] = R.worst(e[i])
    _log(family, prec, c.name, got)
    for k, v in got.items():
        assert v <= R.bar(family, prec, k), (k, v, where.get(k))
    return dqkv


def _head_cols(t, heads, h):
    """the columns of head h of a [rows, parts*heads*64] tensor, as a [rows, parts*64] tensor of its own"""
    rows = t.shape[0]
    return t.view(rows, -1, heads, 64)[:, :, h].reshape(rows, -1).contiguous()


# ---- A: tile seams -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N", R.A_NS)
def test_tile_seams(prec, N):
    """N at and beside the seams (N % 64 crossing 32: the skipped upper half; N % 128 crossing 0: a further workgroup; N crossing 32:
    waves that only stage): O, LSE, dQ, dK, dV per head against fp64; a NaN-filled dqkv is overwritten; two calls agree bit for bit; at
    N in {33, 97, 129} the 16-bit-output twins hold the bits of T(out) and of the backward on the upcast out."""
    c = _cuda(next(x for x in R.cases("A", prec) if x.N == N))
    out, lse = _forward("A", prec, c)
    dqkv = _backward("A", prec, c, out, lse)
    poisoned = torch.full_like(dqkv, float("nan"))
    hip.attention_train_bwd(c.qkv, out, c.dout, lse, c.n, N, c.heads, dq_scale=DQ, dqkv=poisoned)
    assert bool(torch.isfinite(dqkv).all()) and torch.equal(_bits(poisoned), _bits(dqkv))
    out2, lse2 = hip.attention_train_fwd(c.qkv, c.n, N, c.heads)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(_bits(lse2), _bits(lse))
    if N in R.A_TWIN_NS:
        out16, lse16 = hip.attention_train_fwd(c.qkv, c.n, N, c.heads, out_dtype=R.DT[prec])
        assert out16.dtype == R.DT[prec]
        assert torch.equal(_bits(out16), _bits(out.to(R.DT[prec]))) and torch.equal(_bits(lse16), _bits(lse))
        got = hip.attention_train_bwd(c.qkv, out16, c.dout, lse, c.n, N, c.heads, dq_scale=DQ)
        want = hip.attention_train_bwd(c.qkv, out16.float(), c.dout, lse, c.n, N, c.heads, dq_scale=DQ)
        assert torch.equal(_bits(got), _bits(want))


# ---- B: power-of-two homogeneity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_backward_is_homogeneous_in_powers_of_two(prec):
    """bwd(dout 2^k) has the bits of 2^k bwd(dout) for k in {-100, -40, -20, 20, 60, 100} (the scale c takes the 2^k out before anything
    rounds, 1 / c puts it back; the CPU file shows that nothing underflows at these k), and is within the bar against fp64."""
    cs = [_cuda(c) for c in R.cases("B", prec)]
    out, lse = hip.attention_train_fwd(cs[0].qkv, 2, 97, 2)
    base = _backward("B", prec, cs[0], out, lse)
    for c in cs[1:]:
        k = int(c.name[1:])
        got = _backward("B", prec, c, out, lse)
        assert torch.equal(_bits(got), _bits(base * 2.0 ** k)), k


# ---- C: magnitudes per (sequence, head) --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_magnitudes_that_differ_per_head(prec):
    """dout factors 1, 2^-20, 2^-60, 2^40 and 0 over the nine (sequence, head) of n_seq 3, heads 3, N = 65: every head within the bar,
    the zero head exactly zero, and each head's gradients the bits of a heads = 1 call on its own columns."""
    c = _cuda(R.cases("C", prec)[0])
    out, lse = hip.attention_train_fwd(c.qkv, c.n, c.N, c.heads)
    dqkv = _backward("C", prec, c, out, lse)
    zs, zh = R.C_ZERO
    assert bool((dqkv.view(c.n, c.N, 3, c.heads, 64)[zs, :, :, zh] == 0).all())
    for h in range(c.heads):
        alone = hip.attention_train_bwd(_head_cols(c.qkv, c.heads, h), _head_cols(out, c.heads, h), _head_cols(c.dout, c.heads, h),
                                        lse[:, h:h + 1].contiguous(), c.n, c.N, 1, dq_scale=DQ)
        assert torch.equal(_bits(alone), _bits(_head_cols(dqkv, c.heads, h))), h


# ---- D: bottom and top of the range ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_tiny_heads_are_finite_and_accurate(prec):
    """One head with max |dO| = 2^-124, one with 1e-40, two at unit scale: every output finite, the tiny heads within their bars (see
    the header), the unit-scale heads the bits of a run in which the tiny heads are zero."""
    c = _cuda(R.cases("D", prec)[0])
    clean = _cuda(R.cases("D_clean", prec)[0])
    out, lse = hip.attention_train_fwd(c.qkv, c.n, c.N, c.heads)
    raw = hip.attention_train_bwd(c.qkv, out, c.dout, lse, c.n, c.N, c.heads, dq_scale=DQ)
    bad = int((~torch.isfinite(raw)).sum())
    print(f"D {prec}: {bad} of {raw.numel()} gradients are not finite")
    assert bad == 0
    dqkv = _backward("D", prec, c, out, lse, tiny=dict(zip(R.D_TINY, ("2m124", "1em40"))))
    want = hip.attention_train_bwd(clean.qkv, out, clean.dout, lse, c.n, c.N, c.heads, dq_scale=DQ)
    g, w = dqkv.view(c.n, c.N, 3, c.heads, 64), want.view(c.n, c.N, 3, c.heads, 64)
    for s in range(c.n):
        for h in range(c.heads):
            if (s, h) in R.D_TINY:
                assert bool((w[s, :, :, h] == 0).all()) and bool((g[s, :, :, h] != 0).any())
            else:
                assert torch.equal(_bits(g[s, :, :, h]), _bits(w[s, :, :, h])), (s, h)


@pytest.mark.parametrize("prec", PRECS)
def test_inf_and_nan_stay_in_their_head(prec):
    """A single +inf in one head of dout and a single NaN in another: the other heads are the bits of the clean run."""
    n, heads, N = 2, 2, 65
    qkv = R.qkv16(n, heads, N, R.DT[prec], 500).cuda()
    dout = R.dout_scaled(n, heads, N, 501).cuda()
    out, lse = hip.attention_train_fwd(qkv, n, N, heads)
    want = hip.attention_train_bwd(qkv, out, dout, lse, n, N, heads, dq_scale=DQ).view(n, N, 3, heads, 64)
    poisoned = dout.clone().view(n, N, heads, 64)
    poisoned[0, 17, 1, 5] = float("inf")
    poisoned[1, N - 1, 0, 63] = float("nan")
    got = hip.attention_train_bwd(qkv, out, poisoned.view_as(dout), lse, n, N, heads, dq_scale=DQ).view(n, N, 3, heads, 64)
    for s, h in ((0, 0), (1, 1)):
        assert bool(torch.isfinite(got[s, :, :, h]).all()) and torch.equal(_bits(got[s, :, :, h]), _bits(want[s, :, :, h])), (s, h)


# ---- E: score structure ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("family", [f for f in R.FAMILIES if f.startswith("E_")])
def test_score_structure(prec, family):
    """Forward and backward on N = 97, n_seq 2, heads 2 against fp64 on the same rounded operands.
    E_offset0 / 30 / 300: every score of row i shifted by +-t (q_0 = +-1, k_0 += t), which leaves the softmax alone; the LSE bar is
    attn_train_ref.lse_bound, elementwise.  E_dominant: one key leading by about 12 at index 0, 31, 32, 63, 64, 96 (the exact running
    maximum, the upper half of a tile).  E_same_keys: all keys and all values identical -- O is the common v row, LSE = s + ln N, dQ = dK
    = 0 (the reference's, to 1e-12: see the CPU file); like E_dominant's nearly-zero dQ and dK they are taken relative to the head's
    whole gradient.  E_negative: all scores about -200, small spread."""
    for c in R.cases(family, prec):
        c = _cuda(c)
        lse_bar = R.lse_bound(c.qkv, c.n, c.heads, c.N) if family.startswith("E_offset") else None
        out, lse = _forward(family, prec, c, lse_bar)
        _backward(family, prec, c, out, lse)


# ---- F: sparse dO ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_dout_in_one_query_row(prec):
    """dout nonzero in query row 0 only (what the last block of the classifier sees) and in row N-1 only, N in {33, 65, 129}: dK and dV
    are sums over queries, and the padded rows past N re-read row N-1 -- a clone that leaks doubles the answer."""
    for c in R.cases("F", prec):
        c = _cuda(c)
        out, lse = hip.attention_train_fwd(c.qkv, c.n, c.N, c.heads)
        _backward("F", prec, c, out, lse)


# ---- G: fp16 headroom of dS --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prec", PRECS)
def test_large_aligned_v_and_dout_inside_the_envelope(prec):
    """v and dO aligned so that |dP - D| / max |dO| passes 1000: the 16-bit dS = P o c (dP - D) reaches 2^13 (fp16 ends at 2^16; the CPU
    file holds the input below 2^14).  Finite gradients within the bar."""
    c = _cuda(R.cases("G", prec)[0])
    out, lse = hip.attention_train_fwd(c.qkv, c.n, c.N, c.heads)
    dqkv = _backward("G", prec, c, out, lse)
    assert bool(torch.isfinite(dqkv).all())
