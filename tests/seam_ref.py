"""References, bars and constructions shared by tests/test_encoder_seam_gpu.py and tests/test_encoder_seam_cpu.py: the kernels on both sides of
the fused encoder's blocked-layout seam (16-bit attention in the encoder's log2-domain contract, its blocked epilogue, the CLS-row attention,
the QKV GEMM on blocked rows, the token kernel), each against a plain fp64 form of the same operation on the same rounded operands.

Everything here runs on the CPU in torch; nothing imports the HIP library.  u is the unit roundoff of the 16-bit type (2^-8 bf16, 2^-11
fp16): round-to-nearest moves a value by at most u times its magnitude.
"""
import functools
import math

import torch

from mst import synth

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -24}
LOG2E = 1.4426950408889634
QSCALE = 0.125 * LOG2E                        # what mst_vit_encode passes as col_scale for the q columns of a 16-bit QKV projection
GUARD, SENTINEL = 64, 12288.0                 # guard rows behind a buffer and their fill: exact in bf16 and fp16 (tests/test_block_boundary_gpu.py)
E, HID = 384, 1536


def rnd(shape, seed, scale=1.0):
    return torch.from_numpy(synth.hash_normal(tuple(shape), seed, 77)) * scale


def heads_of(qkv, n, N, heads):
    """q, k, v as fp64 [n, heads, N, 64] from the packed rows [n*N, 3*heads*64]."""
    return qkv.double().reshape(n, N, 3, heads, 64).permute(2, 0, 3, 1, 4)


def rows_of(t, n, N, heads):
    return t.transpose(1, 2).reshape(n * N, heads * 64)


def worst_ratio(got, ref, bar):
    """max |got - ref| / bar; an element that is exact counts 0 whatever its bar."""
    err = (got.double().cpu() - ref.double().cpu()).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bar.double().cpu()).max())


# ---- (a) attention in the encoder's contract ------------------------------------------------------------------------------------------
ATTN_SHAPES = [(2, 17, 1), (3, 33, 2), (2, 64, 2), (3, 65, 2), (3, 97, 6), (2, 129, 2), (3, 257, 6), (2, 300, 2), (1, 1370, 6)]


def attn_operands(dt, n, N, heads, seed=30, log2q=True):
    """tests/test_hip_ops.py::test_attention's operands with q scaled ONCE, by 0.35 log2 e, before it is rounded (the encoder's contract)."""
    qkv = rnd((n * N, 3 * heads * 64), seed)
    qkv[:, : heads * 64] *= 0.35 * (LOG2E if log2q else 1.0)
    return qkv.to(DT.get(dt, torch.float32))


def attn_ref2(qkv, n, N, heads):
    """fp64 softmax2(q k^T) v on the stored operands.  Returns (ref [n*N, E], P @ |V| [n*N, E], P [n, heads, N, N], scores)."""
    q, k, v = heads_of(qkv, n, N, heads)
    s = q @ k.transpose(-2, -1)
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    p = p / p.sum(-1, keepdim=True)
    return rows_of(p @ v, n, N, heads), rows_of(p @ v.abs(), n, N, heads), p, s


def attn_bar(ref, mag, N, dt):
    """|got - ref| <= (u + N 2^-23) (P @ |V|) + u |ref|, element by element.  The kernel computes fp32 scores from the stored operands
    (exact products, fp32 sums: inside the N 2^-23 term), p = exp2(s - r) in fp32, rounds p to the operand type for P.V (each p moves by
    at most u p: the u (P @ |V|) term; the row sum is taken from the unrounded p), accumulates P.V and the sum in fp32 over N keys (the
    N 2^-23 term again) and rounds the quotient to the output type (u |ref|).  Nothing else is rounded in this contract."""
    return (U[dt] + N * 2.0 ** -23) * mag + U[dt] * ref.abs()


def emulate_attn(qkv, n, N, heads, dt, below, mutant=None):
    """The kernel's arithmetic with ONE reference point per row, `below` under the row maximum (negative: above it) and rounded to the
    operand type as the kernel's is: fp32 scores, p = exp2(s - r) in fp32, P rounded to 16 bits for P.V, the row sum from the unrounded p,
    the quotient rounded to 16 bits.  mutant: 'drop' / 'double' (the row's heaviest key is left out of / counted twice in P.V), 'truncate'
    (P chopped towards zero instead of rounded), 'sum_rounded' (the row sum taken from the rounded P)."""
    tdt = DT[dt]
    q, k, v = heads_of(qkv, n, N, heads)
    s = (q @ k.transpose(-2, -1)).float()
    r = (s.max(-1, keepdim=True).values - below).to(tdt).float()
    p = torch.exp2(s - r)
    p16 = p.to(tdt)
    if mutant == "truncate":
        bits = 16 if tdt == torch.bfloat16 else 13
        chopped = (p.view(torch.int32) >> bits << bits).view(torch.float32)
        p16 = chopped.to(tdt)                 # (fp16: exact for normal halves, which every p within 2^-14 of the reference point is)
    elif mutant in ("drop", "double"):
        top = p.argmax(-1, keepdim=True)
        p16 = p16.scatter(-1, top, p16.gather(-1, top) * (0.0 if mutant == "drop" else 2.0))
    l = (p16.float() if mutant == "sum_rounded" else p).sum(-1, keepdim=True)
    o = (p16.double() @ v).float()
    return rows_of((o / l).to(tdt), n, N, heads)


def emulate_attn_tiled(qkv, n, N, heads, dt, fast_floor=None):
    """k_attn16.hip's tile loop, every query row taken as its own wave: 64-key tiles, the 16-bit reference point that moves when a tile's
    maximum exceeds it by more than 8, FAST mode (reference 0, no maximum, the tile's row sum as the range guard) behind a first tile
    with |max| <= TH0 (fp16: 0 <= max <= TH0; fast_floor = -8.0 gives fp16's earlier, two-sided entry test), a tripped guard re-running the
    tile the classic way.  fp32 state, 16-bit P."""
    tdt = DT[dt]
    TH0, GUARD_SUM, RT = (8.0, 32768.0, 8.0) if tdt == torch.float16 else (60.0, 1.2676506e30, 8.0)
    floor = (0.0 if tdt == torch.float16 else -TH0) if fast_floor is None else fast_floor
    q, k, v = heads_of(qkv, n, N, heads)
    s = (q @ k.transpose(-2, -1)).float()
    shape = s.shape[:-1] + (1,)
    r, l = torch.zeros(shape), torch.zeros(shape)
    o = torch.zeros(s.shape[:-1] + (64,))
    fast = torch.zeros(shape, dtype=torch.bool)
    nt, nt_full = (N + 63) // 64, N // 64
    for t in range(nt):
        st, vt = s[..., t * 64:(t + 1) * 64], v[..., t * 64:(t + 1) * 64, :]
        if t > 0 and t < nt_full:
            with_sum = torch.exp2(st).sum(-1, keepdim=True)
            fast = fast & (with_sum < GUARD_SUM)             # a tripped guard: classic from here on, the reference point still 0
        elif t > 0:
            fast = torch.zeros_like(fast)                    # the ragged last tile always runs the classic way
        mx = (st - r).max(-1, keepdim=True).values
        if t == 0:
            fast = (mx >= floor) & (mx <= TH0)
        move = ~fast & ((mx > RT) if t else torch.ones_like(fast))
        r_new = torch.where(move, (r + mx).to(tdt).float(), r)
        alpha = torch.ones_like(r) if t == 0 else torch.exp2(-(r_new - r))
        r, l, o = r_new, l * alpha, o * alpha
        p = torch.exp2(st - r)
        l = l + p.sum(-1, keepdim=True)
        o = o + (p.to(tdt).double() @ vt).float()
    return rows_of((o / l).to(tdt), n, N, heads)


# ---- (c) one-hot selection -------------------------------------------------------------------------------------------------------------
ONEHOT_N = [33, 65, 129, 257, 300]


def onehot_case(dt, n, N, heads):
    """qkv whose softmax selects exactly one key per query, and what the attention must return bit for bit.

    Key j carries the 10-bit code of j as +-8 in its first ten dims, query q the code of pi(q) = (a q + b) mod N with gcd(a, N) = 1 and
    its own (a, b) per (sequence, head): the selected key scores 10 * 64 = 640, a key that differs in h bits 640 - 128 h.  Every score is
    a multiple of 128 (exact in fp32, and as a reference point exact in bf16 and fp16), so p is exactly 1 for the selected key and
    2^-128 or less for the others: against v values of magnitude >= 1 they vanish in the fp32 sums.  v holds signed integers of
    magnitude 1 .. 251 (exact in both types), a function of (sequence, head, key, dim) that no two keys of a (sequence, head) share.
    Returns (qkv in dt, expected [n*N, heads*64] in dt, pi [n, heads, N])."""
    assert N <= 1024
    Ew = heads * 64
    code = (((torch.arange(N)[:, None] >> torch.arange(10)[None, :]) & 1) * 16 - 8).float()       # [N, 10] of +-8
    qkv = torch.zeros(n, N, 3, heads, 64)
    pi = torch.zeros(n, heads, N, dtype=torch.long)
    coprime = [a for a in range(3, 4 * N) if math.gcd(a, N) == 1]
    key, d = torch.arange(N)[:, None], torch.arange(64)[None, :]
    for s in range(n):
        for h in range(heads):
            a, b = coprime[(s * heads + h) * 5 % len(coprime)], 7 * s + 3 * h + 1
            pi[s, h] = (a * torch.arange(N) + b) % N
            qkv[s, :, 0, h, :10] = code[pi[s, h]]
            qkv[s, :, 1, h, :10] = code
            mag = 1 + torch.where(d < 32, (key * (d + 1) + 13 * h + 29 * s) % 251, (key * (d + 1) + 13 * h + 29 * s) % 241)
            qkv[s, :, 2, h] = (mag * (1 - 2 * ((key + d) & 1))).float()
    expect = torch.stack([torch.stack([qkv[s, pi[s, h], 2, h] for h in range(heads)], dim=1) for s in range(n)])     # [n, N, heads, 64]
    tdt = DT.get(dt, torch.float32)
    return qkv.reshape(n * N, 3 * Ew).to(tdt), expect.reshape(n * N, Ew).to(tdt), pi


# ---- (d) fp16 FAST mode under low row maxima ---------------------------------------------------------------------------------------------
LOWMAX = dict(n=2, N=300, heads=2)


def lowmax_operands(dt):
    """Small positive q against negative keys: every row's largest log2-score in [-8, -6.5] -- the first tile passes the FAST-mode entry
    test |max| <= 8 of fp16 -- with one key up there and the others about 11 below it.  Under a reference point of 0 those others
    have p near 2^-18: fp16 subnormals once P is rounded for P.V (their errors, up to 2^-25 each against the u p = 2^-29 the bar grants,
    show wherever the one heavy key's v element is small), unless the kernel keeps its reference point near the maximum.  The scores are q_d = a_q, k_d = -b_j (1 + small noise), 64 dims: s = -64 a_q b_j or so."""
    n, N, heads = LOWMAX["n"], LOWMAX["N"], LOWMAX["heads"]
    Ew = heads * 64
    qkv = rnd((n * N, 3 * Ew), 91)
    a = 0.125 * (1 + 0.03 * torch.tanh(rnd((n * N, 1), 92)))                       # a_q in [0.121, 0.129]
    qkv[:, :Ew] = a * (1 + 0.02 * torch.tanh(qkv[:, :Ew]))
    top = torch.arange(N) == 5                                                     # ONE key near the maximum, in the first tile; the others ~11 below it
    b = torch.where(top, torch.full((N,), 0.89), 2.3 + 0.04 * torch.tanh(rnd((N,), 94)))
    kk = -(b.repeat(n)[:, None]) * (1 + 0.02 * torch.tanh(qkv[:, Ew:2 * Ew]))
    qkv[:, Ew:2 * Ew] = kk
    return qkv.to(DT[dt])


def lowmax_constraint(s):
    """The two conditions the issue sets on the fp64 log2-scores s [n, heads, N, N] of the case, as (row maxima in range, smallest share
    of a row's keys that lie 6 to 12 below its maximum)."""
    mx = s.max(-1, keepdim=True).values
    below = mx - s
    share = ((below >= 6) & (below <= 12)).double().mean(-1)
    return bool(((mx >= -8) & (mx <= -6.5)).all()), float(share.min())


# ---- (e) CLS-row attention ---------------------------------------------------------------------------------------------------------------
CLS_SHAPES = [(1, 1, 1), (5, 3, 2), (2, 17, 6), (3, 257, 6), (2, 300, 2)]


def cls_ref(qkv, n, N, heads, log2q):
    """fp64 (out [n, heads*64], P @ |V| likewise, probs [n, heads, N]) of query 0 of every sequence; log2q: the scores are log2-domain."""
    q, k, v = heads_of(qkv, n, N, heads)
    s = q[:, :, :1] @ k.transpose(-2, -1)
    s = s - s.max(-1, keepdim=True).values
    p = torch.exp2(s) if log2q else torch.exp(s)
    p = p / p.sum(-1, keepdim=True)
    return (p @ v).reshape(n, heads * 64), (p @ v.abs()).reshape(n, heads * 64), p[:, :, 0]


# ---- (f) QKV GEMM --------------------------------------------------------------------------------------------------------------------------
GEMM_M = [1, 31, 33, 8192, 2 * 8192 + 7, 3 * 8192 - 1, 11 * 8 * 32 * 4 + 5]


def gemm_bar(ref, dt):
    """tests/test_hip_ops.py::test_gemm_weights_in_registers_qkv_shape's bar: the output rounding on values of magnitude >= 1, plus 1e-3."""
    return U[dt] * ref.abs().clamp_min(1.0) + 1e-3


# ---- (g) token kernel ----------------------------------------------------------------------------------------------------------------------
TOKEN_SHAPES = [(3, 56, 84, 0), (5, 42, 28, 4), (2, 14, 14, 0), (1, 14, 518, 0), (2, 224, 224, 0)]


def token_operands(dt, idt, n, H, W, R):
    """tests/test_hip_ops.py::test_patch_embed's operands: (vol in idt, wp [384, 224] in dt, bias, prefix [1+R, 384], pos [Np, 384])."""
    Np = (H // 14) * (W // 14)
    vol = rnd((n, H, W), 40).to(idt)
    w = rnd((E, 3, 14, 14), 41) / math.sqrt(588)
    wp = torch.zeros(E, 14, 16)
    wp[:, :, :14] = w.sum(1)
    return vol, wp.reshape(E, 224).to(DT[dt]), rnd((E,), 42) * 0.1, rnd((1 + R, E), 43), rnd((Np, E), 44) * 0.2


def token_ref(vol, wp, bias, prefix, pos):
    """fp64 tokens [n, 1+R+Np, 384] on the rounded operands (the pixels are rounded to wp's type before the product, as the kernel does)."""
    n, H, W = vol.shape
    Np = (H // 14) * (W // 14)
    cols = vol.float().reshape(n, H // 14, 14, W // 14, 14).permute(0, 1, 3, 2, 4).reshape(n, Np, 196).to(wp.dtype).double()
    wk = wp.double().reshape(E, 14, 16)[:, :, :14].reshape(E, 196)
    return torch.cat([prefix.double().expand(n, -1, -1), cols @ wk.t() + bias.double() + pos.double()], dim=1)


def plain_layernorm(x, eps=1e-6):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps)


# ---- the block tail (tests/test_block_boundary_gpu.py and the chain replay) -----------------------------------------------------------------
def block_reference(x, att, weights):
    """fp64 block arithmetic (attention.py:67-68; block.py:89-94,112-113; mlp.py:34-40) on x fp32 [M, 384] and the attention rows att
    [M, 384], on their device: (x_out, plain LayerNorm of x_out, max(|proj|, |mlp|) -- the scale the bars on x are relative to).
    weights = (proj_w, proj_b, fc1_w, fc1_b, fc2_w, fc2_b, ln2_w, ln2_b), no LayerScale."""
    wp, bp, w1, b1, w2, b2, g, be = (w.double().to(x.device) for w in weights)
    outs, norms, scale = [], [], 0.0
    for lo in range(0, x.shape[0], 16384):  # row chunks bound the memory of the hidden layer
        xd, ad = x[lo:lo + 16384].double(), att[lo:lo + 16384].double()
        proj = ad @ wp.t() + bp
        xmid = xd + proj
        h = torch.nn.functional.layer_norm(xmid, (E,), g, be, 1e-6)
        h = h @ w1.t() + b1
        h = 0.5 * h * (1 + torch.erf(h / math.sqrt(2)))
        y = h @ w2.t() + b2
        ref = xmid + y
        scale = max(scale, float(y.abs().max()), float(proj.abs().max()))
        outs.append(ref)
        norms.append(torch.nn.functional.layer_norm(ref, (E,)))
    return torch.cat(outs), torch.cat(norms), scale


BLOCK_TOL = {"bf16": 1.5e-2, "fp16": 2.5e-3}   # tests/test_block_boundary_gpu.py: x of the scale above; four times that, absolute, for the normalised rows


@functools.lru_cache(maxsize=16)
def cached(fn, *args):
    """One reference per argument tuple, shared by the tests that need it: leave the tensors unchanged."""
    return fn(*args)
