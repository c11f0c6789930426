"""tests/attn_train_ref.py against itself, on the CPU: the fp64 reference against torch.autograd, the fp32 emulation of the training
attention's rounding points (csrc/k_attn16_train.hip) against the reference on every input family of test_attn_train_range_gpu.py -- its
worst per-head errors are the EMU table the GPU bars come from --, the mutants of the dO scaling that those inputs must catch, the
power-of-two homogeneity the GPU test asserts bit for bit, the per-head metric, and the envelope of the fp16 headroom input."""

import math

import pytest
import torch

import attn_train_ref as R
from test_attn_train_gpu import BWD_BARS

PRECS = list(R.DT)


def _case(family, prec, name=None):
    cs = R.cases(family, prec)
    return cs[0] if name is None else next(c for c in cs if c.name == name)


def _emu_errors(c, policy):
    ref = R.ref_bwd(c.qkv, c.dout, c.n, c.heads, c.N, 0.125)
    return R.head_errors(R.emulate_bwd(c.qkv, c.dout, 0.125, policy, c.n, c.heads, c.N), ref, c.n, c.N, c.heads)


@pytest.mark.parametrize("N", [1, 33, 65])
def test_reference_is_fp64_autograd(N):
    """ref_fwd / ref_bwd (closed form) equal softmax(q k^T) v and its torch.autograd gradients in fp64 to 1e-12 of the largest entry."""
    n, heads = 2, 2
    qkv = R.qkv16(n, heads, N, torch.float16, 900 + N)
    dout = R.dout_scaled(n, heads, N, 901 + N)
    q, k, v = (t.clone().requires_grad_(True) for t in R._split(qkv, n, heads, N, torch.float64))
    s = q @ k.transpose(-1, -2)
    o = torch.softmax(s, dim=-1) @ v
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), R._heads(dout.double(), n, heads, N))
    want = R._pack(gq * 0.125, gk, gv, n, heads, N)
    got = R.ref_bwd(qkv, dout, n, heads, N, 0.125)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    O, L = R.ref_fwd(qkv, n, heads, N)
    assert float((O - R._rows(o.detach(), n, heads, N)).abs().max()) <= 1e-12
    assert float((L - torch.logsumexp(s.detach(), -1)).abs().max()) <= 1e-12


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulation_against_fp64_gives_the_table(family, prec):
    """emulate_fwd / emulate_bwd("pow2_per_head") against fp64 on the family's inputs: the worst per-head errors are the entries of
    R.EMU to 10 % (another BLAS may sum in another order), and they are rounding-sized: no emulated gradient misses by 1."""
    got = R.emulation_errors(family, prec)
    table = R.EMU[family][prec]
    print(family, prec, {k: f"{v:.3g}" for k, v in got.items()})
    assert set(got) == set(table)
    for k, v in got.items():
        assert abs(v - table[k]) <= 0.1 * table[k], (k, v, table[k])
        assert v < 0.25, (k, v)


def test_scale_is_a_finite_normal_power_of_two_over_the_whole_range():
    """pow2_scale, the rule of attn_train_pre_kernel: c and 1 / c are normal fp32 numbers for every finite m > 0, denormals included;
    c m lies in [32, 64) from m = 2^-121 up; c = 1 for 0, inf and beyond 3e38."""
    tiny = torch.finfo(torch.float32).tiny
    m = torch.tensor([2.0 ** e for e in range(-149, 128)] + [1e-40, 1.9e-37, 3.0e38, 1.5 * 2.0 ** -121], dtype=torch.float32)
    c = R.pow2_scale(m)
    assert bool(torch.isfinite(c).all()) and bool((c >= tiny).all()) and bool((1 / c >= tiny).all()) and bool(torch.isfinite(1 / c).all())
    assert bool((torch.frexp(c)[0] == 0.5).all())
    big = m >= 2.0 ** -121
    assert bool(((c * m)[big] >= 32).all()) and bool(((c * m)[big] < 64).all())
    assert bool((c[~big] == 2.0 ** 126).all())
    assert R.pow2_scale(torch.tensor([0.0, float("inf"), 3.3e38])).tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("prec,family,name,policy,bar_family", [
    ("fp16", "B", "k-20", "none", "B"),
    ("fp16", "C", None, "pow2_per_tensor", "C"),
    ("fp16", "B", "k-20", "d_unscaled", "B"),
    ("bf16", "B", "k-20", "d_unscaled", "B"),
])
def test_mutants_miss_the_bar_by_ten_times(prec, family, name, policy, bar_family):
    """Each wrong scaling rule, run through the emulation on the input meant to catch it, has a worst per-head error of at least 10 x
    the GPU bar of that test in at least one of dQ, dK, dV; the kernel's own rule stays below the bar."""
    c = _case(family, prec, name)
    e = _emu_errors(c, policy)
    ratio = [float(e[i].max()) / R.bar(bar_family, prec, t) for i, t in enumerate(R.NAMES)]
    print(prec, family, policy, [f"{r:.3g}" for r in ratio])
    assert max(ratio) >= 10, ratio
    good = _emu_errors(c, "pow2_per_head")
    zero = R.ref_bwd(c.qkv, c.dout, c.n, c.heads, c.N, 0.125).view(c.n, c.N, 3, c.heads, 64).abs().amax((1, 4)).permute(1, 0, 2) == 0
    assert bool((good[zero] == 0).all())
    for i, t in enumerate(R.NAMES):
        assert float(good[i][~zero[i]].max()) < R.bar(bar_family, prec, t)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("k", R.B_KS)
def test_emulation_is_homogeneous_in_powers_of_two(prec, k):
    """emulate_bwd(dout 2^k) == 2^k emulate_bwd(dout) bit for bit at every k of part B: nothing underflows or overflows there."""
    base, c = _case("B", prec, "k0"), _case("B", prec, f"k{k}")
    assert torch.equal(c.dout, base.dout * 2.0 ** k)
    want = R.emulate_bwd(base.qkv, base.dout, 0.125, "pow2_per_head", 2, 2, 97) * 2.0 ** k
    got = R.emulate_bwd(c.qkv, c.dout, 0.125, "pow2_per_head", 2, 2, 97)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_whole_tensor_norm_hides_a_head_and_the_per_head_metric_does_not():
    """The fp64 gradient of the mixed-magnitude table with the 2^-60 head doubled: the whole-tensor relative L2 of the existing tests
    stays below their bar (BWD_BARS), the per-head maximum is 1 and points at that head."""
    c = _case("C", "fp16")
    ref = R.ref_bwd(c.qkv, c.dout, c.n, c.heads, c.N, 0.125)
    s, h = 1, 0
    assert R.C_TABLE[s][h] == 2.0 ** -60
    bad = ref.clone().view(c.n, c.N, 3, c.heads, 64)
    bad[s, :, :, h] *= 2
    bad = bad.view_as(ref)
    whole = [float((bad.view(-1, 3, c.heads * 64)[:, i] - ref.view(-1, 3, c.heads * 64)[:, i]).norm() / ref.view(-1, 3, c.heads * 64)[:, i].norm())
             for i in range(3)]
    e = R.head_errors(bad, ref, c.n, c.N, c.heads)
    print("whole-tensor", whole, "per-head max", float(e.max()))
    assert max(whole) < min(BWD_BARS.values())
    for i in range(3):
        val, where = R.worst(e[i])
        assert abs(val - 1.0) < 1e-12 and where == (s, h)
    assert float(R.head_errors(ref, ref, c.n, c.N, c.heads).max()) == 0.0
    # an exactly-zero reference head: the entry is max |got|; a NaN anywhere in a head gives inf for it
    zs, zh = R.C_ZERO
    bad = ref.clone().view(c.n, c.N, 3, c.heads, 64)
    bad[zs, 3, 1, zh, 5] = 7.0
    bad[0, 0, 2, 0, 0] = float("nan")
    e = R.head_errors(bad.view_as(ref), ref, c.n, c.N, c.heads)
    assert float(e[1, zs, zh]) == 7.0 and math.isinf(float(e[2, 0, 0])) and float(e[0].max()) == 0.0


@pytest.mark.parametrize("prec", PRECS)
def test_headroom_input_stays_inside_the_fp16_envelope(prec):
    """Part G's input: in fp64, max |c dS| per (sequence, head) lies in [2^12, 2^14] -- |dP - D| / max |dO| beyond 1000 somewhere, where
    fp16's dS is within a factor 16 of its largest number, and below 2^14 everywhere, a quarter of it."""
    c = _case("G", prec)
    n, heads, N = c.n, c.heads, c.N
    q, k, v = R._split(c.qkv, n, heads, N, torch.float64)
    do = R._heads(c.dout.double(), n, heads, N)
    p = torch.softmax(q @ k.transpose(-1, -2), -1)
    dp = do @ v.transpose(-1, -2)
    diff = dp - (p * dp).sum(-1, keepdim=True)
    m = c.dout.view(n, N, heads, 64).abs().amax((1, 3))
    cds = (R.pow2_scale(m).double()[..., None, None] * p * diff).abs().amax((-1, -2))
    print(prec, "max |c dS| per head", cds.tolist(), "max |dP - D| / max |dO|", float((diff.abs().amax((-1, -2)) / m).max()))
    assert float(cds.min()) >= 2.0 ** 12 and float(cds.max()) <= 2.0 ** 14
    assert float((diff.abs().amax((-1, -2)) / m).max()) > 1000


@pytest.mark.parametrize("prec", PRECS)
def test_score_structures_are_what_they_claim(prec):
    """Part E's inputs in fp64: the offsets are about 0, 30 and 300 and leave the softmax of the unrounded construction alone (here:
    |LSE| grows by the offset); the dominant key holds more than 0.9 of the median row; identical keys give LSE = s + ln N and O = the
    common v row; the negative scores are about -200 with a spread below 2.  The derived LSE bound holds for the fp32 emulation."""
    for t in R.E_OFFSETS:
        c = _case(f"E_offset{t}", prec)
        _, L = R.ref_fwd(c.qkv, c.n, c.heads, c.N)
        L0 = R.ref_fwd(_case("E_offset0", prec).qkv, c.n, c.heads, c.N)[1]
        sign = torch.tensor([1.0, -1.0], dtype=torch.float64).repeat(c.N)[:c.N]
        assert float((L - L0 - t * sign).abs().max()) < 0.02 * t + 1e-9          # k_0 + t rounds to 16 bits
        _, l = R.emulate_fwd(c.qkv, c.n, c.heads, c.N)
        assert bool(((l.double() - L).abs() <= R.lse_bound(c.qkv, c.n, c.heads, c.N)).all())
    for c in R.cases("E_dominant", prec):
        q, k, _ = R._split(c.qkv, c.n, c.heads, c.N, torch.float64)
        p = torch.softmax(q @ k.transpose(-1, -2), -1)
        assert float(p[..., int(c.name[3:])].median()) > 0.9
    c = _case("E_same_keys", prec)
    q, k, v = R._split(c.qkv, c.n, c.heads, c.N, torch.float64)
    O, L = R.ref_fwd(c.qkv, c.n, c.heads, c.N)
    assert float((L - ((q * k[:, :, :1]).sum(-1) + math.log(c.N))).abs().max()) < 1e-12
    assert float((R._heads(O, c.n, c.heads, c.N) - v[:, :, :1]).abs().max()) < 1e-12
    ref = R.ref_bwd(c.qkv, c.dout, c.n, c.heads, c.N, 0.125).view(-1, 3, c.heads * 64)
    assert float(ref[:, :2].abs().max()) < 1e-12 * float(ref[:, 2].abs().max())
    c = _case("E_negative", prec)
    q, k, _ = R._split(c.qkv, c.n, c.heads, c.N, torch.float64)
    s = q @ k.transpose(-1, -2)
    assert float(s.max()) < -195 and float(s.min()) > -205 and float(s.std()) < 2
