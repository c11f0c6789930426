"""Memory-efficient attention of the mixed-precision training step (csrc/k_attn16_train.hip, train_attention='flash'): the forward with its
per-row log-sum-exp and the FlashAttention-2 backward against fp64 torch on the same 16-bit inputs, the model's gradients against the fp32
and the stored-probability steps, and the memory the stored probabilities no longer take."""

import pytest
import torch

from mst import hip, synth

pytestmark = pytest.mark.gpu

FWD_SHAPES = [(1, 6, 1), (3, 6, 2), (3, 12, 63), (1, 6, 65), (3, 6, 257), (64, 6, 257), (1, 12, 261), (3, 6, 261), (1, 6, 1370),
              (64, 6, 1370), (3, 12, 1370)]
BWD_SHAPES = [(1, 6, 1), (3, 6, 2), (3, 12, 63), (1, 6, 65), (3, 6, 257), (64, 6, 257), (1, 12, 261), (1, 6, 1370), (3, 12, 1370)]
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _qkv16(n, heads, N, dt, seed):
    """Packed q | k | v rows rounded to the 16-bit type; q carries the projection's head_dim^-0.5 and a spread that moves the running
    maximum (score standard deviation 2.5)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n * N, 3, heads, 64, device="cuda", generator=g)
    x[:, 0] *= 0.125 * 2.5
    return x.reshape(n * N, 3 * heads * 64).to(dt).contiguous()


def _split64(qkv16, n, heads, N):
    x = qkv16.double().view(n, N, 3, heads, 64).permute(2, 0, 3, 1, 4)         # [3, n, heads, N, 64]
    return x[0], x[1], x[2]


def _ref_fwd(qkv16, n, heads, N):
    """fp64 O [n*N, heads*64] and LSE [n, heads, N], one sequence at a time (the score tensor of 64 x 6 x 1370 is 5.8 GB in fp64)."""
    q, k, v = _split64(qkv16, n, heads, N)
    O = torch.empty(n, N, heads, 64, dtype=torch.float64, device="cuda")
    L = torch.empty(n, heads, N, dtype=torch.float64, device="cuda")
    for i in range(n):
        s = q[i] @ k[i].transpose(-1, -2)
        L[i] = torch.logsumexp(s, dim=-1)
        O[i] = (torch.softmax(s, dim=-1) @ v[i]).transpose(0, 1)
    return O.view(n * N, heads * 64), L


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("n,heads,N", FWD_SHAPES)
def test_forward_and_lse_against_fp64(prec, n, heads, N):
    """O and LSE of mst_attention_train_fwd against fp64 on the same rounded q, k, v.  The probabilities meet V as 16-bit MFMA operands,
    so O carries one rounding of P; LSE comes from fp32 scores of exact products.  Worst measured on the MI355X over FWD_SHAPES: O rel-L2
    8.9e-5 (fp16) / 7.1e-4 (bf16), LSE 4.2e-6 absolute; the bars are 2x those."""
    qkv = _qkv16(n, heads, N, DT[prec], 1000 + N + heads)
    out, lse = hip.attention_train_fwd(qkv, n, N, heads)
    torch.cuda.synchronize()
    O, L = _ref_fwd(qkv, n, heads, N)
    e_o = _rel(out, O)
    e_l = float((lse.double() - L).abs().max())
    print(f"fwd {prec} n={n} h={heads} N={N}: O rel-L2 {e_o:.3e}, LSE max abs {e_l:.3e}")
    assert e_o < {"fp16": 1.8e-4, "bf16": 1.4e-3}[prec], e_o
    assert e_l < 8.5e-6, e_l


def _ref_bwd(qkv16, dout, n, heads, N, dq_scale):
    """fp64 autograd of O = softmax(q k^T) v per sequence: dqkv [n*N, 3*heads*64] with dQ times dq_scale."""
    q, k, v = _split64(qkv16, n, heads, N)
    do = dout.double().view(n, N, heads, 64).transpose(1, 2)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    for i in range(n):
        qi, ki, vi = (t[i].clone().requires_grad_(True) for t in (q, k, v))
        o = torch.softmax(qi @ ki.transpose(-1, -2), dim=-1) @ vi
        gq, gk, gv = torch.autograd.grad(o, (qi, ki, vi), do[i])
        dq[i], dk[i], dv[i] = gq * dq_scale, gk, gv
    return torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(n * N, 3 * heads * 64)


# 2x the worst relative L2 error measured on the MI355X over BWD_SHAPES (any of dQ, dK, dV; N >= 2): fp16 4.27e-4 (dQ, N = 65),
# bf16 5.58e-3 (dQ, N = 2)
BWD_BARS = {"fp16": 8.5e-4, "bf16": 1.1e-2}


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("n,heads,N", BWD_SHAPES)
def test_backward_against_fp64_autograd(prec, n, heads, N):
    """dQ, dK, dV of mst_attention_train_bwd against fp64 autograd on the same rounded q, k, v and the same dO, dq_scale = 0.125: relative
    L2 per tensor below BWD_BARS.  Also: two calls give identical bits, every element of a poisoned dqkv is written."""
    n_e = 3 * heads * 64
    qkv = _qkv16(n, heads, N, DT[prec], 2000 + N + heads)
    g = torch.Generator(device="cuda").manual_seed(7 + N)
    dout = torch.randn(n * N, heads * 64, device="cuda", generator=g)
    out, lse = hip.attention_train_fwd(qkv, n, N, heads)
    dqkv = hip.attention_train_bwd(qkv, out, dout, lse, n, N, heads, dq_scale=0.125)
    torch.cuda.synchronize()
    ref = _ref_bwd(qkv, dout, n, heads, N, 0.125).view(n * N, 3, heads * 64)
    got = dqkv.view(n * N, 3, heads * 64)
    # N = 1: one key, P = 1, so the exact dQ and dK are 0 -- their error is taken relative to the whole gradient's norm instead
    # (measured 2.2e-4 fp16, 1.2e-3 bf16)
    den = [float(ref.double().norm()) if N == 1 and i < 2 else float(ref[:, i].double().norm()) for i in range(3)]
    errs = [float((got[:, i].double() - ref[:, i].double()).norm()) / den[i] for i in range(3)]
    print(f"bwd {prec} n={n} h={heads} N={N}: dQ {errs[0]:.3e} dK {errs[1]:.3e} dV {errs[2]:.3e}")
    assert max(errs) < BWD_BARS[prec], errs
    again = hip.attention_train_bwd(qkv, out, dout, lse, n, N, heads, dq_scale=0.125)
    assert torch.equal(again, dqkv)
    poisoned = torch.full((n * N, n_e), float("nan"), device="cuda")
    hip.attention_train_bwd(qkv, out, dout, lse, n, N, heads, dq_scale=0.125, dqkv=poisoned)
    assert torch.equal(poisoned, dqkv)


def test_bad_arguments_raise():
    qkv = _qkv16(2, 6, 5, torch.bfloat16, 3)
    out, lse = hip.attention_train_fwd(qkv, 2, 5, 6)
    dout = torch.randn_like(out)
    with pytest.raises(TypeError):
        hip.attention_train_fwd(qkv.float(), 2, 5, 6)
    with pytest.raises(ValueError):
        hip.attention_train_fwd(qkv, 2, 6, 6)                                  # shape does not match n_seq * N rows
    with pytest.raises(ValueError):
        hip.attention_train_bwd(qkv, out, dout, lse[:, :, :4].contiguous(), 2, 5, 6)
    with pytest.raises(ValueError):
        hip.attention_train_bwd(qkv, out.half(), dout, lse, 2, 5, 6)
    with pytest.raises(RuntimeError, match="head_dim"):
        hip.attention_train_fwd(qkv.view(10, 3 * 12 * 32), 2, 5, 12, head_dim=32)
    lib = hip.load()
    s = hip.stream_of(qkv)
    assert lib.mst_attention_train_fwd(hip.ptr(qkv), hip.F32, 2, 5, 6, 64, hip.ptr(out), hip.ptr(lse), s) == 1
    assert "dtype" in hip.last_error()
    assert lib.mst_attention_train_fwd(hip.ptr(qkv), hip.BF16, 2, 0, 6, 64, hip.ptr(out), hip.ptr(lse), s) == 1
    nb = lib.mst_attention_train_bwd_workspace_bytes(2, 5, 6, 64)
    assert nb > 0 and lib.mst_attention_train_bwd_workspace_bytes(2, 5, 6, 32) == 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    dq = torch.empty(10, 3 * 6 * 64, device="cuda")
    args = (hip.ptr(qkv), hip.BF16, hip.ptr(out), hip.ptr(dout), hip.ptr(lse), 2, 5, 6, 64, 1.0, hip.ptr(dq))
    assert lib.mst_attention_train_bwd(*args, hip.ptr(ws), nb - 1, s) == 1              # short workspace
    assert "workspace" in hip.last_error()
    assert lib.mst_attention_train_bwd(*args, hip.ptr(ws), nb, s) == 0
    assert lib.mst_attention_train_bwd(*args[:8], 32, *args[9:], hip.ptr(ws), nb, s) == 1


# ---- the training step -------------------------------------------------------------------------------------------------------------

def _grads(build, src, tgt):
    m = build().cuda().train()
    logits = m(src)
    torch.nn.functional.cross_entropy(logits, tgt).backward()
    return logits.detach(), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}


def _compare(a, b):
    la, ga = a
    lb, gb = b
    assert set(ga) == set(gb)
    worst = max(_rel(ga[k], gb[k]) for k in gb)
    glob = (sum(float((ga[k] - gb[k]).double().square().sum()) for k in gb) / sum(float(gb[k].double().square().sum()) for k in gb)) ** 0.5
    return float((la - lb).abs().max()), worst, glob


def _dino(prec, attn, size="s", **kw):
    from mst.models import DinoV2ClassifierSlice

    def build():
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, model_size=size, train_precision=prec, train_attention=attn, **kw)
        m.load_state_dict(synth.synth_state_dict(size, 0))
        return m
    return build


def _dino_reg(prec, attn):
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT

    def build():
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_registers=True, train_precision=prec,
                                  train_attention=attn)
        m.encoder = _ViT(384, 12, 6, img_size=224, num_register_tokens=4, layerscale=1.0, chunked=False)
        m.load_state_dict(synth.synth_state_dict("s", 23, img_size=224, layerscale=True, chunked=False, num_register_tokens=4), strict=True)
        return m
    return build


# (builder, size, precision, bars against the fp32 step (per parameter, global), bars against the stored mixed step (per parameter, global)).
# Against the fp32 step: the bars of test_mixed_precision_step_gradients_against_the_fp32_step.  Against the stored step: 2x the worst
# measured on the MI355X -- flash vs stored, per parameter / global: s_fp16 5.8e-3 / 4.3e-3, s_bf16 6.3e-2 / 3.0e-2, reg261_fp16
# 4.6e-3 / 3.3e-3, vitb_fp16 3.8e-3 / 2.5e-3 (flash vs fp32: 5.6e-3 / 4.0e-3, 3.5e-2 / 2.7e-2, 5.5e-3 / 3.9e-3, 4.5e-3 / 3.3e-3).
STEP_CASES = {
    "s_fp16": (_dino, "s", "fp16", (1e-2, 8e-3), (1.1e-2, 8.5e-3)),
    "s_bf16": (_dino, "s", "bf16", (1.3e-1, 7e-2), (1.25e-1, 6e-2)),
    "reg261_fp16": (_dino_reg, None, "fp16", (1e-2, 8e-3), (9e-3, 6.5e-3)),
    "vitb_fp16": (_dino, "b", "fp16", (1e-2, 8e-3), (7.5e-3, 5e-3)),
}


@pytest.mark.parametrize("case", list(STEP_CASES))
def test_flash_step_gradients_against_the_fp32_and_stored_steps(case):
    """train_attention='flash' at (1, 1, 4, 224, 224): logits and every parameter gradient against the fp32 step, with the bars of
    test_mixed_precision_step_gradients_against_the_fp32_step (fp16 1e-2 per parameter / 8e-3 global rel-L2, bf16 1.3e-1 / 7e-2), and
    against the 'stored' mixed step of the same precision.  Cases: ViT-S in both precisions, ViT-S with 4 register tokens (N = 261) and
    ViT-B (12 heads)."""
    mk, size, prec, bar32, bar_st = STEP_CASES[case]
    build = (lambda p, a: mk(p, a, size)) if size else mk
    src = synth.synth_volume((1, 1, 4, 224, 224), 3).cuda()
    tgt = torch.tensor([1]).cuda()
    flash = _grads(build(prec, "flash"), src, tgt)
    stored = _grads(build(prec, "stored"), src, tgt)
    full = _grads(build("fp32", "stored"), src, tgt)
    d32, w32, g32 = _compare(flash, full)
    dst, wst, gst = _compare(flash, stored)
    _, wref, gref = _compare(stored, full)
    print(f"{case}: flash vs fp32 logits {d32:.2e} worst {w32:.2e} global {g32:.2e} | flash vs stored logits {dst:.2e} worst {wst:.2e} "
          f"global {gst:.2e} | stored vs fp32 worst {wref:.2e} global {gref:.2e}")
    assert d32 < bar32[0] and w32 < bar32[0] and g32 < bar32[1], (d32, w32, g32)
    assert dst < bar_st[0] and wst < bar_st[0] and gst < bar_st[1], (dst, wst, gst)


def test_flash_step_stores_no_probabilities():
    """Peak memory of one bf16 training step at (1, 1, 8, 518, 518): the stored mode keeps 12 blocks x [8, 6, 1370, 1370] fp32
    probabilities (4.3 GB); the flash mode's peak must be lower by at least 3/4 of that."""
    src = synth.synth_volume((1, 1, 8, 518, 518), 5).cuda()
    tgt = torch.tensor([0]).cuda()
    peaks = {}
    for attn in ("stored", "flash"):
        m = _dino("bf16", attn)().cuda().train()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        torch.nn.functional.cross_entropy(m(src), tgt).backward()
        torch.cuda.synchronize()
        peaks[attn] = torch.cuda.max_memory_allocated()
        del m
        torch.cuda.empty_cache()
    n, heads, N = 8, 6, 1370
    need = 0.75 * 12 * n * heads * N * N * 4
    print(f"peak GiB: stored {peaks['stored'] / 2**30:.2f}, flash {peaks['flash'] / 2**30:.2f}; saved {(peaks['stored'] - peaks['flash']) / 1e9:.2f} GB, "
          f"need {need / 1e9:.2f} GB")
    assert peaks["stored"] - peaks["flash"] >= need
