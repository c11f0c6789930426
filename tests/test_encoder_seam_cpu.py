"""The host side of tests/test_encoder_seam_gpu.py, without a GPU: the C ABI declares and exports the four entry points that expose the
fused encoder's seam kernels (additively: the ABI version is unchanged), their bindings refuse wrong operands before the library is
reached, and the constructions and the bar that the GPU tests rest on are checked against an emulation of the kernel's arithmetic."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import seam_ref as S
from mst import hip

ROOT = Path(__file__).resolve().parents[1]
NEW = {"mst_attention_ex": 9, "mst_attention_cls": 9, "mst_gemm16_blocked": 12, "mst_patch_rows16": 14}


def test_header_declares_and_library_exports_the_seam_entry_points():
    header = (ROOT / "include" / "mst_hip.h").read_text()
    lib = ctypes.CDLL(str(hip.LIB_PATH))
    for sym, nargs in NEW.items():
        m = re.search(rf"^int\s+{sym}\s*\(([^;]*)\)\s*;", header, flags=re.M)
        assert m, f"include/mst_hip.h does not declare {sym}"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert len(args) == nargs == len(hip.SIGNATURES[sym][1]), sym
        assert args[0].startswith("const void*") and args[-1].startswith("mst_stream_t"), sym
        assert hasattr(lib, sym), f"{sym} is not exported"
    assert "MST_ATTN_LOG2Q = 1" in header and "MST_ATTN_OUT_BLOCKED = 2" in header
    assert (hip.ATTN_LOG2Q, hip.ATTN_OUT_BLOCKED) == (1, 2)
    lib.mst_version.restype = ctypes.c_int
    assert lib.mst_version() == 300 == hip.ABI_VERSION


def test_encoder_still_calls_the_launchers_directly():
    """The entry points forward to the launchers; mst_vit_encode does not go through them."""
    api = (ROOT / "new-vit_amd" / "csrc" / "mst_api.hip").read_text()
    body = api[api.index("struct vit_call"):api.index("// ---- across-slice transformer + head")]
    for sym in NEW:
        assert sym not in body, sym
    for launcher in ("launch_attn16(", "launch_gemm16_wreg(", "launch_patch_rows16(", "launch_cls_attn("):
        assert launcher in body, launcher


def test_bindings_reject_bad_operands_before_the_library():
    qkv = torch.zeros(2 * 17, 3 * 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="HIP device"):                    # host tensors
        hip.attention(qkv, 2, 17, 1, log2q=True)
    with pytest.raises(ValueError, match="HIP device"):
        hip.attention(qkv, 2, 17, 1, out_blocked=True)
    with pytest.raises(TypeError, match="float32"):                        # the log2-domain and blocked forms are 16-bit only
        hip.attention(qkv.float(), 2, 17, 1, log2q=True)
    with pytest.raises(ValueError, match=r"must be \[34, 384\], got \[34, 192\]"):
        hip.attention(qkv, 2, 17, 2, log2q=True)
    with pytest.raises(ValueError, match="head_dim"):
        hip.attention(qkv, 2, 17, 1, 32, log2q=True)
    with pytest.raises(TypeError):
        hip.attention(qkv.float().numpy(), 2, 17, 1, log2q=True)
    with pytest.raises(ValueError, match="HIP device"):
        hip.attention_cls(qkv, 2, 17, 1)
    with pytest.raises(TypeError):
        hip.attention_cls(qkv.double(), 2, 17, 1)
    with pytest.raises(ValueError, match=r"must be \[32, 192\], got \[34, 192\]"):
        hip.attention_cls(qkv, 2, 16, 1)
    with pytest.raises(ValueError):
        hip.attention_cls(qkv, 0, 17, 1)

    a, w, b = torch.zeros(64, 384, dtype=torch.float16), torch.zeros(1152, 384, dtype=torch.float16), torch.zeros(1152)
    with pytest.raises(ValueError, match="HIP device"):
        hip.gemm_blocked(a, 40, w, b)
    with pytest.raises(TypeError, match="a_blocked is torch.float32"):
        hip.gemm_blocked(a.float(), 40, w, b)
    with pytest.raises(ValueError, match="whole 32-row groups"):           # 40 rows are no whole groups
        hip.gemm_blocked(a[:40], 40, w, b)
    with pytest.raises(ValueError, match="whole 32-row groups"):           # more rows than the buffer holds
        hip.gemm_blocked(a, 65, w, b)
    with pytest.raises(ValueError, match="whole 32-row groups"):
        hip.gemm_blocked(torch.zeros(64, 768, dtype=torch.float16), 40, w, b)

    vol, wp = torch.zeros(2, 28, 42), torch.zeros(384, 224, dtype=torch.bfloat16)
    bias, prefix, pos = torch.zeros(384), torch.zeros(1, 384), torch.zeros(6, 384)
    with pytest.raises(ValueError, match="HIP device"):
        hip.patch_rows16(vol, wp, bias, prefix, pos)
    with pytest.raises(TypeError, match="wp is torch.float32"):            # the fused pipeline is 16-bit only
        hip.patch_rows16(vol, wp.float(), bias, prefix, pos)
    with pytest.raises(ValueError, match="multiples of 14"):
        hip.patch_rows16(torch.zeros(2, 28, 40), wp, bias, prefix, pos)
    with pytest.raises(ValueError, match=r"pos_patch must be \[6, 384\]"):
        hip.patch_rows16(vol, wp, bias, prefix, torch.zeros(5, 384))
    with pytest.raises(ValueError, match=r"wp must be \[384, 224\]"):
        hip.patch_rows16(vol, torch.zeros(384, 196, dtype=torch.bfloat16), bias, prefix, pos)
    with pytest.raises(TypeError):
        hip.patch_rows16(vol.double(), wp, bias, prefix, pos)


def test_blocked_layout_helpers_round_trip_and_match_the_kernel_epilogue_addresses():
    """from_blocked16 against the address arithmetic of the attention epilogue (k_attn16.hip) written out element by element: feature
    f = 64 h + 32 db + 8 g + 4 h2 + e of row R at (R >> 5) * 32 E + 4 h * 512 + (R & 31) * 8 + 4 h2 + db * 1024 + (g >> 1) * 512 + (g & 1) * 256 + e."""
    heads, rows = 2, 96
    Ew = heads * 64
    a = torch.arange(rows * Ew, dtype=torch.float32).reshape(rows, Ew)
    blk = hip.to_blocked16(a).reshape(-1)
    assert torch.equal(hip.from_blocked16(blk.reshape(rows, Ew)), a)
    for R in (0, 31, 32, 95):
        for h in range(heads):
            for db in range(2):
                for g in range(4):
                    for h2 in range(2):
                        for e in range(4):
                            f = 64 * h + 32 * db + 8 * g + 4 * h2 + e
                            off = (R >> 5) * 32 * Ew + 4 * h * 512 + (R & 31) * 8 + 4 * h2 + db * 1024 + (g >> 1) * 512 + (g & 1) * 256 + e
                            assert blk[off] == a[R, f], (R, f)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("N", S.ONEHOT_N)
def test_onehot_construction_selects_exactly(dt, N):
    n, heads = 2, 2
    qkv, expect, pi = S.onehot_case(dt, n, N, heads)
    assert torch.equal(qkv.float().to(qkv.dtype), qkv)                     # every operand is exact in the type
    q, k, v = S.heads_of(qkv, n, N, heads)
    s = q @ k.transpose(-2, -1)
    assert bool((s % 128 == 0).all()) and float(s.max()) == 640
    assert torch.equal(s.argmax(-1), pi) and bool(((s == 640).sum(-1) == 1).all())
    assert float(torch.where(s == 640, torch.full_like(s, -1e9), s).max()) <= 512
    assert len({(a, b) for a, b in zip(pi[:, :, 0].flatten().tolist(), pi[:, :, 1].flatten().tolist())}) == n * heads   # its own (a, b) per (sequence, head)
    assert float(v.abs().min()) >= 1 and float(v.abs().max()) <= 251
    for s_ in range(n):
        for h in range(heads):
            assert len({tuple(r) for r in v[s_, h].tolist()}) == N                                # no two keys share a v row
    if N > 64:                                                                                   # both kinds of query exist: selected key in tile 0 / in a later tile
        assert bool((pi < 64).any()) and bool((pi >= 64).any())
    if dt != "fp32":
        got = S.emulate_attn_tiled(qkv, n, N, heads, dt)
        assert torch.equal(got, expect)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n,N,heads", [(2, 17, 1), (3, 65, 2), (2, 129, 2), (2, 300, 2)])
def test_attention_bar_holds_for_the_kernel_arithmetic_and_catches_mutants(dt, n, N, heads):
    """The bar of seam_ref.attn_bar against an emulation of the kernel's arithmetic (fp32 scores and exp2, 16-bit P, the row sum of
    the unrounded p) at reference points from 8 below the row maximum up to it -- where the classic loop keeps it: inside the bar.
    A dropped or double-counted key and a P that is chopped instead of rounded are outside it.  Taking the row sum from the ROUNDED P
    is not: the rounding errors of P largely cancel between numerator and denominator, the mutant stays inside the bar and this
    suite cannot tell it from the kernel."""
    qkv = S.attn_operands(dt, n, N, heads)
    ref, mag, _, _ = S.attn_ref2(qkv, n, N, heads)
    bar = S.attn_bar(ref, mag, N, dt)
    worst = max(S.worst_ratio(S.emulate_attn(qkv, n, N, heads, dt, below), ref, bar) for below in (0.0, 2.5, 5.0, 8.0))
    ratios = {m: S.worst_ratio(S.emulate_attn(qkv, n, N, heads, dt, 3.0, m), ref, bar) for m in ("drop", "double", "truncate", "sum_rounded")}
    print(f"{dt} {(n, N, heads)}: kernel arithmetic {worst:.3f} of the bar; mutants " + ", ".join(f"{m} {r:.2f}" for m, r in ratios.items()))
    assert worst < 1.0
    assert ratios["drop"] > 10 and ratios["double"] > 10
    assert ratios["truncate"] > 1.0
    assert ratios["sum_rounded"] < 1.0        # not distinguishable (see the docstring)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_lowmax_case_meets_its_constraint_and_what_the_emulation_predicts(dt):
    """The operands of the fp16 FAST-mode case: the constraint of the GPU test holds on the rounded operands, and the emulations show what
    is at stake -- with the reference point near the maximum both types are inside the bar, with fp16's reference point left at 0 (7 or so
    above these maxima, where FAST mode left it while fp16 entered it on |max| <= 8: 2.189 of the bar in this emulation and, to the
    digit, on MI355X) the rounded P falls into fp16's subnormals and the result leaves the bar.  fp16 now enters FAST mode on
    0 <= max <= 8 only."""
    n, N, heads = S.LOWMAX["n"], S.LOWMAX["N"], S.LOWMAX["heads"]
    qkv = S.lowmax_operands(dt)
    ref, mag, _, s = S.attn_ref2(qkv, n, N, heads)
    in_range, share = S.lowmax_constraint(s)
    assert in_range and share >= 0.25, (in_range, share)
    assert bool((s[..., :64].max(-1).values.abs() <= 8).all())             # the first tile passes fp16's FAST-mode entry test
    bar = S.attn_bar(ref, mag, N, dt)
    near = S.worst_ratio(S.emulate_attn(qkv, n, N, heads, dt, 0.0), ref, bar)
    far = S.worst_ratio(S.emulate_attn(qkv, n, N, heads, dt, -7.25), ref, bar)
    tiled = S.worst_ratio(S.emulate_attn_tiled(qkv, n, N, heads, dt), ref, bar)
    two_sided = S.worst_ratio(S.emulate_attn_tiled(qkv, n, N, heads, dt, fast_floor=-8.0), ref, bar)
    print(f"{dt}: share {share:.2f}; reference at the maximum {near:.3f}, 7.25 above it {far:.3f}, the kernel's tile loop {tiled:.3f}, "
          f"the tile loop with FAST mode entered on |max| <= 8 {two_sided:.3f} of the bar")
    assert near < 1.0 and tiled < 1.0
    if dt == "bf16":
        assert far < 1.0                                                   # fp32's exponent range: the reference point does not matter
    else:
        assert far > 2.0 and two_sided > 2.0                               # the case tells a reference point left 7 above the maxima from one near them
