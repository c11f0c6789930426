"""Reference, emulation, inputs and metric for the dynamic-range tests of the training attention (csrc/k_attn16_train.hip):
tests/test_attn_train_range_cpu.py checks this file against itself on the CPU, tests/test_attn_train_range_gpu.py holds the kernels to it.
Plain torch, no GPU needed; every function works on the device of its arguments.

  ref_fwd / ref_bwd          fp64 O, LSE and dQ * dq_scale, dK, dV from the rounded 16-bit qkv and the fp32 dout (closed form)
  emulate_fwd / emulate_bwd  fp32 models of the kernels' rounding points; the GPU bars are 4x their worst per-head error (EMU below)
  head_errors                relative L2 per (sequence, head) and tensor -- a whole-tensor norm hides one wrong head among many
  cases(family, prec)        the seeded inputs of every family, built on the CPU so that both test files see the same bits

`python tests/attn_train_ref.py` prints the EMU table from the emulation (the CPU test fails when the table no longer matches it)."""

from collections import namedtuple

import torch

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
U32 = 2.0 ** -24                                                                 # unit roundoff of fp32

# ---- layouts ---------------------------------------------------------------------------------------------------------------------------


def _split(qkv16, n, heads, N, dtype):
    x = qkv16.to(dtype).view(n, N, 3, heads, 64).permute(2, 0, 3, 1, 4)          # [3, n, heads, N, 64]
    return x[0], x[1], x[2]


def _heads(rows, n, heads, N):
    """[n*N, heads*64] -> [n, heads, N, 64]"""
    return rows.view(n, N, heads, 64).permute(0, 2, 1, 3)


def _rows(x, n, heads, N):
    """[n, heads, N, 64] -> [n*N, heads*64]"""
    return x.permute(0, 2, 1, 3).reshape(n * N, heads * 64)


def _pack(dq, dk, dv, n, heads, N):
    return torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(n * N, 3 * heads * 64)


# ---- fp64 reference ----------------------------------------------------------------------------------------------------------------------

def ref_fwd(qkv16, n, heads, N):
    """fp64 O [n*N, heads*64] and LSE [n, heads, N] (natural log) of softmax(q k^T) v on the rounded operands."""
    q, k, v = _split(qkv16, n, heads, N, torch.float64)
    s = q @ k.transpose(-1, -2)
    return _rows(torch.softmax(s, dim=-1) @ v, n, heads, N), torch.logsumexp(s, dim=-1)


def ref_bwd(qkv16, dout, n, heads, N, dq_scale):
    """fp64 dqkv [n*N, 3*heads*64] (dQ times dq_scale) of O = softmax(q k^T) v for the fp32 dout: dV = P^T dO, dP = dO V^T,
    dS = P o (dP - rowsum(P o dP)), dQ = dS K, dK = dS^T Q."""
    q, k, v = _split(qkv16, n, heads, N, torch.float64)
    do = _heads(dout.double(), n, heads, N)
    p = torch.softmax(q @ k.transpose(-1, -2), dim=-1)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    return _pack(ds @ k * dq_scale, ds.transpose(-1, -2) @ q, p.transpose(-1, -2) @ do, n, heads, N)


# ---- fp32 emulation of the kernels' rounding points --------------------------------------------------------------------------------------

def emulate_fwd(qkv16, n, heads, N):
    """fp32 O and LSE as attn_train_fwd_kernel rounds them: fp32 scores of exact 16-bit products, times log2 e, p = 2^(s - max) in fp32,
    the probabilities rounded to T where they meet V, O times the rounded reciprocal of the fp32 sum of the unrounded p, LSE = (max + log2 sum) ln 2.
    Not modelled: the running maximum per 64-key tile, the MFMA accumulation order, v_exp_f32 / v_log_f32 against exp2 / log2."""
    T = qkv16.dtype
    q, k, v = _split(qkv16, n, heads, N, torch.float32)
    s2 = (q @ k.transpose(-1, -2)) * LOG2E
    m = s2.amax(-1, keepdim=True)
    p = torch.exp2(s2 - m)
    l = p.sum(-1, keepdim=True)
    o = (p.to(T).float() @ v) * (1.0 / l)
    return _rows(o, n, heads, N), ((m + torch.log2(l)) * LN2).squeeze(-1)


def pow2_scale(m):
    """The preprocess kernel's c for m = max |dO| (fp32 tensor): 2^min(6 - e, 126) with m in [2^(e-1), 2^e), so c m in [32, 64) down to
    m = 2^-121 and c = 2^126 below; 1 for m == 0 and m > 3e38."""
    ok = (m > 0) & (m <= 3.0e38)
    e = torch.where(ok, torch.frexp(torch.where(ok, m, torch.ones_like(m)))[1], 0)
    return torch.where(ok, torch.ldexp(torch.ones_like(m), torch.clamp(6 - e, max=126)), torch.ones_like(m))


SCALE_POLICIES = ("pow2_per_head", "none", "pow2_per_tensor", "d_unscaled")


def emulate_bwd(qkv16, dout, dq_scale, scale_policy, n, heads, N, out=None, lse=None):
    """fp32 model of attn_train_pre_kernel / attn_train_dkv_kernel / attn_train_dq_kernel per (sequence, head): c from scale_policy,
    do16 = T(c dO), D = c rowsum(dO o O), P = exp(S - LSE), dP = do16 V^T, dS = T(P o (dP - D)), P16 = T(P), dV = P16^T do16 / c,
    dK = dS^T q / c, dQ = dq_scale dS k / c.  out / lse default to emulate_fwd's.  scale_policy: "pow2_per_head" is the kernel's rule;
    the mutants are "none" (c = 1), "pow2_per_tensor" (one c from the whole tensor's maximum) and "d_unscaled" (the kernel's c, D not
    multiplied by it)."""
    assert scale_policy in SCALE_POLICIES, scale_policy
    T = qkv16.dtype
    q, k, v = _split(qkv16, n, heads, N, torch.float32)
    if out is None:
        out, lse = emulate_fwd(qkv16, n, heads, N)
    do = _heads(dout.float(), n, heads, N)
    o = _heads(out.float(), n, heads, N)
    a = torch.nan_to_num(do.abs(), nan=0.0, posinf=float("inf"))                 # the kernel's fmaxf skips NaN
    if scale_policy == "none":
        c = torch.ones(n, heads, dtype=torch.float32, device=do.device)
    elif scale_policy == "pow2_per_tensor":
        c = pow2_scale(a.amax()).expand(n, heads)
    else:
        c = pow2_scale(a.amax((-1, -2)))
    c = c[..., None, None]
    do16 = (do * c).to(T).float()
    D = (do * o).sum(-1, keepdim=True)
    if scale_policy != "d_unscaled":
        D = D * c
    p = torch.exp(q @ k.transpose(-1, -2) - lse.float()[..., None])
    ds = (p * (do16 @ v.transpose(-1, -2) - D)).to(T).float()
    p16 = p.to(T).float()
    ic = 1.0 / c
    dqs = torch.tensor(dq_scale, dtype=torch.float32, device=do.device) / c      # exact: c is a power of two
    return _pack((ds @ k) * dqs, (ds.transpose(-1, -2) @ q) * ic, (p16.transpose(-1, -2) @ do16) * ic, n, heads, N)


# ---- metric ----------------------------------------------------------------------------------------------------------------------------

def head_errors(got, want, n_seq, N, heads, whole=()):
    """Relative L2 error per tensor and (sequence, head): [t, n_seq, heads] fp64 for got / want [n_seq*N, t*heads*64] (t = 3: dQ, dK,
    dV of a dqkv; t = 1: O).  Where the reference of a (tensor, sequence, head) is exactly zero the entry is max |got| there (the tests
    require 0).  Tensors listed in `whole` are taken relative to the norm of the head's whole gradient instead (an exact reference of
    zero or nearly zero, as dQ and dK with one key).  A non-finite `got` gives inf."""
    t = got.shape[1] // (heads * 64)
    g = got.double().view(n_seq, N, t, heads, 64)
    w = want.double().view(n_seq, N, t, heads, 64)
    num = (g - w).square().sum((1, 4)).sqrt()                                    # [n_seq, t, heads]
    den = w.square().sum((1, 4)).sqrt()
    err = torch.where(den > 0, num / den.clamp_min(1e-300), g.abs().amax((1, 4)))
    for i in whole:
        err[:, i] = num[:, i] / w.square().sum((1, 2, 4)).sqrt()
    return torch.nan_to_num(err, nan=float("inf"), posinf=float("inf")).permute(1, 0, 2).contiguous()


def worst(err):
    """(maximum, its (sequence, head)) of one tensor's [n_seq, heads] errors."""
    i = int(err.argmax())
    return float(err.flatten()[i]), (i // err.shape[1], i % err.shape[1])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def qkv32(n, heads, N, seed):
    """The distribution of test_attn_train_gpu._qkv16 before rounding, [n*N, 3, heads, 64] fp32: i.i.d. normal, q times head_dim^-0.5
    and a spread that moves the running maximum (score standard deviation 2.5)."""
    x = torch.randn(n * N, 3, heads, 64, generator=_gen(seed))
    x[:, 0] *= 0.125 * 2.5
    return x


def _round(x, dt):
    return x.reshape(x.shape[0], -1).to(dt).contiguous()


def qkv16(n, heads, N, dt, seed):
    return _round(qkv32(n, heads, N, seed), dt)


def dout_scaled(n, heads, N, seed, k=0):
    """randn * 2^k"""
    return torch.randn(n * N, heads * 64, generator=_gen(seed)) * 2.0 ** k


def dout_mixed(n, heads, N, seed, table):
    """randn times table[sequence][head]"""
    f = torch.tensor(table, dtype=torch.float64).view(n, 1, heads, 1)
    return (torch.randn(n * N, heads * 64, generator=_gen(seed)).double().view(n, N, heads, 64) * f).float().view(n * N, heads * 64)


def dout_one_row(n, heads, N, seed, row):
    """zero except query row `row` of every sequence"""
    d = torch.zeros(n, N, heads * 64)
    d[:, row] = torch.randn(n, heads * 64, generator=_gen(seed))
    return d.view(n * N, heads * 64)


def dout_head_max(dout, n, heads, N, targets):
    """dout with head (seq, h) rescaled so that its max |dO| is targets[(seq, h)] (0: the head zeroed)"""
    d = dout.double().view(n, N, heads, 64).clone()
    for (s, h), t in targets.items():
        d[s, :, h] *= t / float(d[s, :, h].abs().max())
    return d.float().view(n * N, heads * 64)


Case = namedtuple("Case", "name n heads N qkv dout")

A_NS = (31, 32, 33, 64, 96, 97, 127, 128, 129, 160, 161)
A_TWIN_NS = (33, 97, 129)
B_KS = (-100, -40, -20, 20, 60, 100)
C_TABLE = ((1.0, 2.0 ** -20, 2.0 ** 40), (2.0 ** -60, 0.0, 1.0), (2.0 ** 40, 2.0 ** -20, 2.0 ** -60))
C_ZERO = (1, 1)
D_TINY = {(0, 1): 2.0 ** -124, (1, 0): 1e-40}
E_OFFSETS = (0, 30, 300)
E_DOMINANT = (0, 31, 32, 63, 64, 96)
F_NS = (33, 65, 129)


def _e_qkv(kind, arg, dt):
    """Score structures on N = 97, n_seq 2, heads 2.  Dimension 0 of the head is the handle: q_0 = +-1 makes k_0 a score offset."""
    n, heads, N = 2, 2, 97
    x = qkv32(n, heads, N, 600).view(n, N, 3, heads, 64)
    if kind == "offset":                                                          # row i: every score shifts by q_i0 * t = +-t
        x[:, 0::2, 0, :, 0] = 1.0
        x[:, 1::2, 0, :, 0] = -1.0
        x[:, :, 1, :, 0] += float(arg)
    elif kind == "dominant":                                                      # key `arg` leads every row by about 12: P within 1e-2 of one-hot
        x[:, :, 0, :, 0] = 1.0
        x[:, arg, 1, :, 0] = 12.0
    elif kind == "same_keys":                                                     # one k row and one v row per (sequence, head)
        x[:, :, 1:] = x[:, :1, 1:]
    elif kind == "negative":                                                      # scores about -200, standard deviation 0.5
        x[:, :, 0] *= 0.2
        x[:, :, 0, :, 0] = 1.0
        x[:, :, 1, :, 0] = -200.0
    return _round(x.reshape(n * N, 3, heads, 64), dt)


def _g_case(dt):
    """fp16 headroom of dS: v and dO aligned with one +-1 pattern w, v_j = a_j w and dO_i = b_i (w + noise), so that dP_ij = dO_i . v_j
    is 64 a_j b_i: the fp64 max |c dS| lies in [2^12, 2^14] (checked in the CPU file), a quarter of fp16's largest number at the most."""
    n, heads, N = 2, 2, 97
    g = _gen(800)
    x = qkv32(n, heads, N, 801).view(n, N, 3, heads, 64)
    w = torch.where(torch.rand(64, generator=g) < 0.5, -1.0, 1.0)
    x[:, :, 2] = torch.randn(n, N, heads, 1, generator=g) * 5.0 * w
    d = (torch.randn(n, N, heads, 1, generator=g).sign() * (w + 0.1 * torch.randn(n, N, heads, 64, generator=g)))
    return Case("G", n, heads, N, _round(x.reshape(n * N, 3, heads, 64), dt), d.reshape(n * N, heads * 64).contiguous())


def cases(family, prec):
    """The inputs of one family (the keys of EMU) as a list of Case, on the CPU."""
    dt = DT[prec]
    if family == "A":
        return [Case(f"N{N}", 2, 2, N, qkv16(2, 2, N, dt, 100 + N), dout_scaled(2, 2, N, 200 + N)) for N in A_NS]
    if family == "B":
        q = qkv16(2, 2, 97, dt, 300)
        return [Case(f"k{k}", 2, 2, 97, q, dout_scaled(2, 2, 97, 301, k)) for k in (0,) + B_KS]
    if family == "C":
        return [Case("mixed", 3, 3, 65, qkv16(3, 3, 65, dt, 400), dout_mixed(3, 3, 65, 401, C_TABLE))]
    if family in ("D", "D_clean"):
        tiny = D_TINY if family == "D" else {k: 0.0 for k in D_TINY}
        return [Case(family, 2, 2, 65, qkv16(2, 2, 65, dt, 500), dout_head_max(dout_scaled(2, 2, 65, 501), 2, 2, 65, tiny))]
    if family.startswith("E_"):
        d = dout_scaled(2, 2, 97, 601)
        if family.startswith("E_offset"):
            t = int(family[len("E_offset"):])
            return [Case(family, 2, 2, 97, _e_qkv("offset", t, dt), d)]
        if family == "E_dominant":
            return [Case(f"key{j}", 2, 2, 97, _e_qkv("dominant", j, dt), d) for j in E_DOMINANT]
        return [Case(family, 2, 2, 97, _e_qkv(family[2:], None, dt), d)]
    if family == "F":
        return [Case(f"N{N}_row{r}", 2, 2, N, qkv16(2, 2, N, dt, 700 + N), dout_one_row(2, 2, N, 701 + N, r)) for N in F_NS for r in (0, N - 1)]
    if family == "G":
        return [_g_case(dt)]
    raise KeyError(family)


FAMILIES = ("A", "B", "C", "D", "E_offset0", "E_offset30", "E_offset300", "E_dominant", "E_same_keys", "E_negative", "F", "G")
# identical keys: the exact dQ and dK are zero; a dominant key: nearly zero (dS = P o (dP - D) cancels).  Both relative to the whole gradient
WHOLE = {"E_same_keys": (0, 1), "E_dominant": (0, 1)}
NAMES = ("dQ", "dK", "dV")


def lse_bound(qkv16, n, heads, N):
    """Absolute bound [n, heads, N] on the kernel's LSE error, from fp32's unit roundoff u = 2^-24 alone.  LSE_i = (m + log2 l) ln 2
    with m = max_j s_ij log2 e and l = sum_j 2^(s_ij log2 e - m):
      * s_ij: 64 exact products summed in fp32, each addition within u of a partial sum that is at most A_i = max_j sum_d |q_id k_jd|:
        64 u A_i;
      * s log2 e, m + log2 l, (.) ln 2 and the two rounded constants: five roundings of a number of LSE's size, and the subtraction
        s_ij log2 e - m, which errs by u |s_ij - m| only where the term no longer counts: 6 u |LSE_i| with that slack;
      * l: at most N terms in [0, 1], each exponential within 2 u, each of the N additions within u l: a relative error of l of
        (N + 2) u, the same absolute error of ln l; the logarithm itself 2 u more.
    In all u (64 A_i + 6 |LSE_i| + N + 4).  With a score offset that dominates, A_i is |LSE_i| to within the spread of the scores, so
    the bar is proportional to |LSE|."""
    q, k, _ = _split(qkv16, n, heads, N, torch.float64)
    A = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1)
    L = torch.logsumexp(q @ k.transpose(-1, -2), dim=-1)
    return U32 * (64 * A + 6 * L.abs() + N + 4)


def emulation_errors(family, prec):
    """Worst per-head error of the emulation against fp64 over the family's cases: {"O", "LSE" (max abs), "dQ", "dK", "dV"}.  Heads
    whose reference is exactly zero (their emulated gradient is too) do not count.  Family D also returns its tiny heads on their own."""
    res = {}

    def up(key, val):
        res[key] = max(res.get(key, 0.0), float(val))

    for c in cases(family, prec):
        n, heads, N = c.n, c.heads, c.N
        O, L = ref_fwd(c.qkv, n, heads, N)
        o, l = emulate_fwd(c.qkv, n, heads, N)
        up("O", head_errors(o, O, n, N, heads).max())
        up("LSE", (l.double() - L).abs().max())
        ref = ref_bwd(c.qkv, c.dout, n, heads, N, 0.125)
        e = head_errors(emulate_bwd(c.qkv, c.dout, 0.125, "pow2_per_head", n, heads, N), ref, n, N, heads, WHOLE.get(family, ()))
        zero = ref.double().view(n, N, 3, heads, 64).abs().amax((1, 4)).permute(1, 0, 2) == 0
        e = torch.where(zero, torch.zeros_like(e), e)
        if family == "D":
            for (s, h), name in zip(D_TINY, ("2m124", "1em40")):
                for i, t in enumerate(NAMES):
                    up(f"{t}_{name}", e[i, s, h])
                e[:, s, h] = 0
        for i, t in enumerate(NAMES):
            up(t, e[i].max())
    return res


# The emulation's worst per-head errors (emulation_errors above, torch on the CPU).  The GPU bars are 4 x these.
EMU = {
    "A": {
        "fp16": {"O": 0.000107, "LSE": 3.89e-06, "dQ": 0.000559, "dK": 0.00053, "dV": 0.000329},
        "bf16": {"O": 0.000864, "LSE": 1.6e-06, "dQ": 0.00413, "dK": 0.00399, "dV": 0.00252},
    },
    "B": {
        "fp16": {"O": 0.000108, "LSE": 2.44e-06, "dQ": 0.000466, "dK": 0.000423, "dV": 0.000308},
        "bf16": {"O": 0.000815, "LSE": 8.98e-07, "dQ": 0.00303, "dK": 0.00289, "dV": 0.0024},
    },
    "C": {
        "fp16": {"O": 0.000102, "LSE": 2e-06, "dQ": 0.000468, "dK": 0.000449, "dV": 0.000298},
        "bf16": {"O": 0.000807, "LSE": 1.57e-06, "dQ": 0.0039, "dK": 0.0041, "dV": 0.00262},
    },
    "D": {
        "fp16": {"O": 9.18e-05, "LSE": 2.7e-06, "dQ_2m124": 0.000469, "dK_2m124": 0.000427, "dV_2m124": 0.000301, "dQ_1em40": 0.0004, "dK_1em40": 0.000391, "dV_1em40": 0.000289, "dQ": 0.000456, "dK": 0.00043, "dV": 0.000292},
        "bf16": {"O": 0.000743, "LSE": 1.36e-06, "dQ_2m124": 0.00351, "dK_2m124": 0.00321, "dV_2m124": 0.00251, "dQ_1em40": 0.00331, "dK_1em40": 0.00316, "dV_1em40": 0.00239, "dQ": 0.00349, "dK": 0.00341, "dV": 0.00235},
    },
    "E_offset0": {
        "fp16": {"O": 0.000104, "LSE": 2.04e-06, "dQ": 0.000422, "dK": 0.000402, "dV": 0.000293},
        "bf16": {"O": 0.000847, "LSE": 1.4e-06, "dQ": 0.00342, "dK": 0.00327, "dV": 0.00249},
    },
    "E_offset30": {
        "fp16": {"O": 0.00011, "LSE": 1.47e-05, "dQ": 0.00161, "dK": 0.000395, "dV": 0.000306},
        "bf16": {"O": 0.000827, "LSE": 8.53e-06, "dQ": 0.0145, "dK": 0.00364, "dV": 0.00248},
    },
    "E_offset300": {
        "fp16": {"O": 0.000122, "LSE": 0.000142, "dQ": 0.0156, "dK": 0.000412, "dV": 0.000304},
        "bf16": {"O": 0.000833, "LSE": 0.000167, "dQ": 0.136, "dK": 0.00361, "dV": 0.00247},
    },
    "E_dominant": {
        "fp16": {"O": 2.9e-05, "LSE": 1.04e-05, "dQ": 0.000412, "dK": 0.000617, "dV": 0.000333},
        "bf16": {"O": 0.000219, "LSE": 5.21e-06, "dQ": 0.00323, "dK": 0.00503, "dV": 0.00275},
    },
    "E_same_keys": {
        "fp16": {"O": 1.52e-08, "LSE": 2.32e-06, "dQ": 0.00261, "dK": 0.000561, "dV": 0.000337},
        "bf16": {"O": 1.52e-08, "LSE": 1.12e-06, "dQ": 0.0211, "dK": 0.00532, "dV": 0.00225},
    },
    "E_negative": {
        "fp16": {"O": 0.000219, "LSE": 2.95e-05, "dQ": 0.00973, "dK": 0.000324, "dV": 0.00034},
        "bf16": {"O": 0.00173, "LSE": 2.42e-05, "dQ": 0.0754, "dK": 0.00249, "dV": 0.00267},
    },
    "F": {
        "fp16": {"O": 0.000107, "LSE": 2.55e-06, "dQ": 0.007, "dK": 0.0061, "dV": 0.000368},
        "bf16": {"O": 0.000815, "LSE": 1.59e-06, "dQ": 0.0206, "dK": 0.0181, "dV": 0.0033},
    },
    "G": {
        "fp16": {"O": 9.03e-05, "LSE": 1.77e-06, "dQ": 0.000221, "dK": 0.000219, "dV": 0.000341},
        "bf16": {"O": 0.000729, "LSE": 1.33e-06, "dQ": 0.00194, "dK": 0.00187, "dV": 0.00272},
    },
}


def bar(family, prec, name):
    return 4.0 * EMU[family][prec][name]


if __name__ == "__main__":
    print("EMU = {")
    for fam in FAMILIES:
        print(f'    "{fam}": {{')
        for prec in DT:
            print(f'        "{prec}": {{' + ", ".join(f'"{k}": {v:.3g}' for k, v in emulation_errors(fam, prec).items()) + "},")
        print("    },")
    print("}")
