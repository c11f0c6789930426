"""The kernels on both sides of the fused encoder's blocked-layout seam, one at a time, on a real MI355X (``-m gpu``).

``mst_vit_encode``'s 16-bit pipeline runs four kernels and kernel modes that no other entry point used to reach: the attention kernel
in the log2-domain contract and with the blocked epilogue, the QKV GEMM that reads blocked rows, the token kernel that also writes
block 0's normalised rows, and the CLS-row attention of ``prune_last_block``.  Through the encoder they are only seen from 12,288 tokens
up and only through CLS embeddings, where one wrong row is diluted by 1/N.  Here each runs through its own entry point
(``mst_attention_ex``, ``mst_attention_cls``, ``mst_gemm16_blocked``, ``mst_patch_rows16``) at shapes of a few hundred rows, against the
plain fp64 form of the same operation on the same rounded operands (tests/seam_ref.py); the last test replays a whole fused encode
from these pieces and holds it to the encoder bit for bit.

Bit-equalities asserted here were predicted from the code before they were run; what each run showed stands in the test's docstring.
"""
import pytest
import torch

import seam_ref as S
from mst import synth

pytestmark = pytest.mark.gpu

DT = S.DT


@pytest.fixture(scope="module")
def hip():
    from mst import hip as h
    h.load()
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return h


def guarded(rows, cols, tdt):
    """`rows` rows and GUARD more behind them, all SENTINEL."""
    return torch.full((rows + S.GUARD, cols), S.SENTINEL, dtype=tdt, device="cuda")


def sentinel(t):
    return bool((t.float() == S.SENTINEL).all())


def blocked_call(hip, qkv, n, N, heads, log2q=True):
    """The attention with the blocked epilogue into a poisoned buffer: (the decoded rows [n*N, E], the buffer, its whole-group row count)."""
    M, Ew = n * N, heads * 64
    Mp = (M + 31) // 32 * 32
    buf = guarded(Mp, Ew, qkv.dtype)
    assert hip.attention(qkv, n, N, heads, log2q=log2q, out_blocked=True, out=buf) is buf
    torch.cuda.synchronize()
    return hip.from_blocked16(buf[:Mp]), buf, Mp


def assert_blocked_equals(hip, qkv, n, N, heads, row_major):
    """(b) the blocked epilogue only changes addresses: the decoded rows are the row-major result bit for bit, and neither the padding rows
    of the last 32-row group nor the guard rows behind it are written (the kernel stores rows q < N only)."""
    M = n * N
    dec, buf, Mp = blocked_call(hip, qkv, n, N, heads)
    assert torch.equal(dec[:M], row_major), "blocked epilogue differs from the row-major one"
    assert sentinel(dec[M:]), "padding rows of the last 32-row group written"
    assert sentinel(buf[Mp:]), "guard rows behind the blocked buffer written"


# ---- (a) + (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n,N,heads", S.ATTN_SHAPES)
def test_attention_encoder_contract(hip, dt, n, N, heads):
    """log2q = 1: q was scaled by head_dim^-0.5 log2 e once, before its only rounding, and the kernel takes exp2 of q.k as stored.  Against
    fp64 softmax2(q k^T) v element by element at seam_ref.attn_bar, (u + N 2^-23) (P @ |V|) + u |ref|: a bar derived from the roundings the
    contract contains, not from a run (test_encoder_seam_cpu.py holds an emulation of the kernel's arithmetic to it, <= 0.92, and shows
    which mutants it catches).  The stand-alone contract of ``test_attention`` rounds q log2 e a second time and has no such bar.
    Shapes: 32-key half-tile skips (17, 33, 97), whole 64-key tiles (64), one key past a tile (65, 129, 257), 32-query waves and
    128-query workgroups (129, 257, 300, 1370), n_seq * N no multiple of 32 (all but 2 x 64).  The row-major result also has 64 guard
    rows behind it; the blocked epilogue is held to it bit for bit (predicted from k_attn16.hip:318-334: one `op` base and three
    strides differ, the values do not).

    Worst ratio to the bar measured on MI355X: 0.893 in bf16 (3 x 257, 6 heads), 0.895 in fp16 (3 x 65, 2 heads); 0.64 - 0.90 over the
    18 cases.  Blocked == row-major bit for bit, padding and guard rows untouched: held in all 18."""
    tdt = DT[dt]
    qkv = S.cached(S.attn_operands, dt, n, N, heads)
    ref, mag, _, _ = S.cached(S.attn_ref2, qkv, n, N, heads)
    M, Ew = n * N, heads * 64
    buf = guarded(M, Ew, tdt)
    got = hip.attention(qkv.cuda(), n, N, heads, log2q=True, out=buf)[:M]
    torch.cuda.synchronize()
    ratio = S.worst_ratio(got, ref, S.attn_bar(ref, mag, N, dt))
    print(f"attention log2q {dt} {(n, N, heads)}: worst error {ratio:.3f} of the bar")
    assert sentinel(buf[M:]), "guard rows behind the row-major output written"
    assert_blocked_equals(hip, qkv.cuda(), n, N, heads, got)
    assert ratio <= 1.0


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("N", S.ONEHOT_N)
def test_attention_onehot_selection_is_bit_exact(hip, dt, N):
    """seam_ref.onehot_case: every query selects exactly one key (score 640, every other at most 512, all multiples of 128), so the output
    row must BE that key's v row, bit for bit: a wrong key, a wrong head or sequence, a row stored at another row's address or a query
    fragment read from the wrong row all show as a wrong integer.  For N > 64 most selected keys lie behind tile 0 (asserted): the
    reference point moves there and what tile 0 accumulated is rescaled by exp2(-128) or less.  Row-major and blocked; the fp32 kernel
    (``mst_attention``, q not in the log2 domain: exp(-128) vanishes as well) must be exact too.

    Held on MI355X in all 15 cases, row-major and blocked."""
    n, heads = 2, 2
    qkv, expect, pi = S.cached(S.onehot_case, dt, n, N, heads)
    if N > 64:
        assert bool((pi >= 64).any()) and bool((pi < 64).any())
    if dt == "fp32":
        got = hip.attention(qkv.cuda(), n, N, heads)
        assert torch.equal(got.cpu(), expect)
        return
    got = hip.attention(qkv.cuda(), n, N, heads, log2q=True)
    wrong = (got.cpu() != expect).any(-1).nonzero().flatten().tolist()
    assert not wrong, f"rows {wrong[:8]} of {n * N} are not their selected key's v row"
    assert_blocked_equals(hip, qkv.cuda(), n, N, heads, got)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_attention_fast_mode_low_row_maxima(hip, dt):
    """Row maxima in [-8, -6.5] of the log2 domain, one key up there and the others about 11 below it (seam_ref.lowmax_operands; the
    constraint is asserted on the fp64 scores before the kernel runs).  An fp16 kernel that enters FAST mode on |max| <= 8 leaves its
    reference point at 0: every p is then at most 2^-6.5 and the keys 11 below the maximum are rounded to fp16 subnormals before P.V, where the
    classic loop -- reference point within 8 of the maximum -- loses nothing down to 14 below it.  The kernel's comment promises that both
    modes agree up to rounding, so the bar is that of test_attention_encoder_contract with no allowance; bf16 has fp32's exponent
    range and must pass as it is.  The emulation of test_encoder_seam_cpu.py puts fp16 with the reference point left at 0 at 2.2 - 2.4
    times the bar and at 0.90 with the reference point at the maximum.

    Worst ratio to the bar measured on MI355X: bf16 0.889.  fp16 2.189 while the kernel entered FAST mode on |max| <= 8 (the
    emulation's figure to the digit); 0.899 since it enters on 0 <= max <= 8 only (k_attn16.hip), the emulation's figure for a
    reference point at the maximum."""
    n, N, heads = S.LOWMAX["n"], S.LOWMAX["N"], S.LOWMAX["heads"]
    qkv = S.cached(S.lowmax_operands, dt)
    ref, mag, _, s = S.cached(S.attn_ref2, qkv, n, N, heads)
    in_range, share = S.lowmax_constraint(s)
    assert in_range and share >= 0.25, (in_range, share)
    got = hip.attention(qkv.cuda(), n, N, heads, log2q=True)
    ratio = S.worst_ratio(got, ref, S.attn_bar(ref, mag, N, dt))
    print(f"attention low maxima {dt}: worst error {ratio:.3f} of the bar")
    assert_blocked_equals(hip, qkv.cuda(), n, N, heads, got)
    assert ratio <= 1.0


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,log2q", [("fp32", False), ("fp16", False), ("fp16", True), ("bf16", False), ("bf16", True)])
@pytest.mark.parametrize("n,N,heads", S.CLS_SHAPES)
def test_attention_cls_rows(hip, dt, log2q, n, N, heads):
    """``mst_attention_cls`` (the `attn_out` branch of cls_probs_kernel, what prune_last_block runs): the CLS query's output and
    probabilities against fp64.  The kernel is fp32 throughout (fp32 dot products, exp, sums; only the output is rounded), so out lies
    within u_out |ref| + 1e-5 (p @ |v|) -- the second term is the project's 1e-5 bar on the probabilities carried through p.v -- and probs
    at that 1e-5 bar.  probs = None is accepted and changes nothing; in the encoder's contract row 0 of the full attention agrees with
    the same reference at the bar of test_attention_encoder_contract.  A single token, fewer keys than the 4 key ranges of the
    output sum (3), a ragged 32-key pass (17, 257, 300).

    Worst ratio to the out bar measured on MI355X: 0.977 (bf16, log2q, 2 x 17, 6 heads); 0.85 - 0.98 for the 16-bit types, 0.05 for fp32
    (the bar's 1e-5 term is generous for an fp32 kernel: it is the project's bar on the probabilities, which measured 2.3e-7 at worst)."""
    tdt = DT.get(dt, torch.float32)
    qkv = S.cached(S.attn_operands, dt, n, N, heads, 33, log2q)
    ref, mag, p = S.cached(S.cls_ref, qkv, n, N, heads, log2q)
    out, probs = hip.attention_cls(qkv.cuda(), n, N, heads, log2q=log2q)
    out2, none = hip.attention_cls(qkv.cuda(), n, N, heads, log2q=log2q, probs=False)
    assert none is None and torch.equal(out, out2)
    assert out.dtype == tdt and out.shape == (n, heads * 64) and probs.shape == (n, heads, N)
    ratio = S.worst_ratio(out, ref, S.U[dt] * ref.abs() + 1e-5 * mag)
    perr = float((probs.double().cpu() - p).abs().max() / p.abs().max())
    print(f"attention_cls {dt} log2q={int(log2q)} {(n, N, heads)}: out {ratio:.3f} of the bar, probs {perr:.2e} (bar 1e-5)")
    assert ratio <= 1.0
    assert perr < 1e-5
    assert torch.allclose(probs.sum(-1).cpu(), torch.ones(n, heads), atol=1e-5)
    if log2q:
        full = hip.attention(qkv.cuda(), n, N, heads, log2q=True).reshape(n, N, heads * 64)[:, 0]
        assert S.worst_ratio(full, ref, S.attn_bar(ref, mag, N, dt)) <= 1.0


# ---- (f) ----------------------------------------------------------------------------------------------------------------------------------
def gemm_operands(dt, M):
    g = torch.Generator().manual_seed(M * 7 + 1152)
    a = torch.randn(M, 384, generator=g).to(DT[dt])
    w = (torch.randn(1152, 384, generator=g) / 384 ** 0.5).to(DT[dt])
    b = torch.randn(1152, generator=g)
    return a, w, b


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("M", S.GEMM_M)
def test_qkv_gemm_on_blocked_rows(hip, monkeypatch, dt, M):
    """``gemm16_wreg_kernel<T, BLK = true>`` (K = 384, N = 1152, the q columns times 0.125 log2 e as the encoder passes them): the rows
    arrive in the blocked layout, the padding rows of the last 32-row group hold NaN -- the kernel reads them (whole groups are
    allocated) and, rows being independent, nothing of them may reach a valid row.  Against the fp64 product at the bar of
    ``test_gemm_weights_in_registers_qkv_shape``; guard rows behind M come back untouched.  M: CUs with 0 to 4 chunks (the counted-vmcnt
    prologue and the vmcnt(0) tail), ragged last chunk; below 8,192 rows the kernel is reached with MST_GEMM_WREG_MIN_M=1.
    Predicted from k_gemm16_wreg.hip: bit-equal to the row-major instantiation on the same operands -- BLK changes the LDS-DMA source
    offsets and the fragment read addresses only; both multiply the same A fragments with the same weight registers in the same k order
    and share the epilogue.

    Worst ratio to the fp64 bar measured on MI355X: 0.936 in bf16, 0.661 in fp16.  Blocked == row-major bit for bit: held in all 14 cases."""
    monkeypatch.setenv("MST_GEMM_WREG_MIN_M", "1")
    tdt = DT[dt]
    a, w, b = gemm_operands(dt, M)
    Mp = (M + 31) // 32 * 32
    ap = torch.cat([a, torch.full((Mp - M, 384), float("nan"), dtype=tdt)]).cuda()
    ab = hip.to_blocked16(ap)
    w, b = w.cuda(), b.cuda()
    full = guarded(M, 1152, tdt)
    got = hip.gemm_blocked(ab, M, w, b, col_scale=S.QSCALE, scale_cols=384, out=full[:M])
    torch.cuda.synchronize()
    ref = a.cuda().double() @ w.double().t() + b.double()
    ref[:, :384] *= float(torch.tensor(S.QSCALE, dtype=torch.float32))
    assert bool(torch.isfinite(got).all()), "a padding row's NaN reached a valid row"
    ratio = S.worst_ratio(got, ref, S.gemm_bar(ref, dt))
    print(f"blocked QKV GEMM {dt} M={M}: worst error {ratio:.3f} of the bar")
    assert ratio <= 1.0
    assert sentinel(full[M:]), "rows behind M written"
    row_major = hip.gemm(a.cuda(), w, b, col_scale=S.QSCALE, scale_cols=384)
    assert torch.equal(got, row_major), "blocked-A and row-major instantiations differ"


def test_qkv_gemm_on_blocked_rows_refuses_other_shapes(hip, monkeypatch):
    """No other kernel reads blocked rows: a shape the weights-in-registers router does not take is an error, never a wrong result."""
    a = torch.zeros(64, 384, dtype=torch.bfloat16, device="cuda")
    w, b = torch.zeros(1152, 384, dtype=torch.bfloat16, device="cuda"), torch.zeros(1152, device="cuda")
    out = guarded(40, 1152, torch.bfloat16)
    monkeypatch.delenv("MST_GEMM_WREG_MIN_M", raising=False)
    with pytest.raises(RuntimeError, match="weights-in-registers"):        # fewer than 8,192 rows
        hip.gemm_blocked(a, 40, w, b, out=out[:40])
    monkeypatch.setenv("MST_GEMM_WREG_MIN_M", "1")
    with pytest.raises(RuntimeError, match="weights-in-registers"):        # the scaled columns end inside a 384-column tile
        hip.gemm_blocked(a, 40, w, b, col_scale=0.5, scale_cols=100, out=out[:40])
    with pytest.raises(RuntimeError, match="weights-in-registers"):        # N no multiple of 384
        hip.gemm_blocked(a, 40, w[:1024], b[:1024], out=None)
    torch.cuda.synchronize()
    assert sentinel(out)


# ---- (g) ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,idt", [("bf16", torch.float32), ("fp16", torch.float32), ("bf16", torch.bfloat16), ("fp16", torch.float16)])
@pytest.mark.parametrize("n,H,W,R", S.TOKEN_SHAPES)
def test_token_kernel_rows(hip, dt, idt, n, H, W, R):
    """``patch_rows16_kernel`` + ``prefix_rows_ln_kernel``: the fp32 residual stream and block 0's plain-normalised rows in one pass.  x
    against the fp64 reference of ``test_patch_embed`` at its 2e-5 of max|ref|; xn against the fp64 plain LayerNorm (eps 1e-6, no
    affine) of the kernel's OWN x -- the stage is checked from its real input -- within u |ref| + 2e-5: the output rounding plus fp32
    statistics.  Shapes: a ragged last 32-patch chunk (72, 30 and 37 patches), chunks that straddle slices, register rows, a one-patch
    grid (two patches in all: one chunk of 2), 16 x 16 grids; fp32 and 16-bit volumes.

    Worst measured on MI355X: x 2.3e-7 of max|ref|; xn 0.993 of its bar in bf16 (2 x 224 x 224), 0.975 in fp16."""
    vol, wp, bias, prefix, pos = S.cached(S.token_operands, dt, idt, n, H, W, R)
    ref = S.cached(S.token_ref, vol, wp, bias, prefix, pos)
    x, xn = hip.patch_rows16(vol.cuda(), wp.cuda(), bias.cuda(), prefix.cuda(), pos.cuda())
    Np = (H // 14) * (W // 14)
    assert x.shape == xn.shape == (n, 1 + R + Np, 384) and x.dtype == torch.float32 and xn.dtype == DT[dt]
    err_x = float((x.double().cpu() - ref).abs().max() / ref.abs().max())
    refn = S.plain_layernorm(x.cpu())
    ratio_n = S.worst_ratio(xn, refn, S.U[dt] * refn.abs() + 2e-5)
    print(f"token kernel {dt} vol {idt} {(n, H, W, R)}: x {err_x:.2e} of max|ref| (bar 2e-5), xn {ratio_n:.3f} of its bar")
    assert err_x < 2e-5
    assert ratio_n <= 1.0
    assert torch.equal(x[:, : 1 + R].cpu(), prefix.expand(n, -1, -1))                      # prefix rows verbatim


# ---- (h) ----------------------------------------------------------------------------------------------------------------------------------
def _model(dt):
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=dt)
    model.encoder = _ViT(384, 3, 6)
    model.load_state_dict(synth.synth_state_dict("s", 17, depth=3), strict=True)
    return model.cuda().eval()


def _chain(hip, model, vol, dt, blocked):
    """One fused encode rebuilt from the op wrappers, as mst_vit_encode chains the launchers (csrc/mst_api.hip): the token kernel; block 0:
    row-major folded QKV, attention, block; blocks 1, 2: QKV, attention, block; final LayerNorm of the CLS rows.  blocked: the encoder's
    layouts (16-bit rows blocked from block 0's attention on, x as the fp32 image between blocks); otherwise everything row-major.
    The weights are built as dino.py's _prepare builds them.  Returns the CLS rows and, per layer, what every stage read and wrote
    (decoded to row-major)."""
    tdt = DT[dt]
    dev = vol.device
    enc = model.encoder
    n, N, heads = vol.shape[0], 1 + 256, 6
    M = n * N
    Mp = (M + 31) // 32 * 32
    f32 = lambda t: t.detach().to(dev, torch.float32)
    with torch.no_grad():
        w = f32(enc.patch_embed.proj.weight)
        wp = torch.zeros(384, 14, 16, device=dev)
        wp[:, :, :14] = w.sum(dim=1)
        wp = wp.reshape(384, 224).to(tdt).contiguous()
        pos = f32(enc.pos_embed[0]).contiguous()
        prefix = (f32(enc.cls_token)[0] + pos[:1]).contiguous()
        x0, xn0 = hip.patch_rows16(vol, wp, f32(enc.patch_embed.proj.bias).contiguous(), prefix, pos[1:].contiguous())
        x = torch.zeros(Mp, 384, device=dev)
        xn = torch.zeros(Mp, 384, dtype=tdt, device=dev)
        x[:M], xn[:M] = x0.reshape(M, 384), xn0.reshape(M, 384)
        stages = []
        for l, b in enumerate(enc.block_list()):
            g1, be1, wq = f32(b.norm1.weight), f32(b.norm1.bias), f32(b.attn.qkv.weight)
            wqf = (wq * g1[None, :]).to(tdt).contiguous()
            bqf = (f32(b.attn.qkv.bias) + (wq * be1[None, :]).sum(dim=1)).contiguous()
            raw = tuple(f32(t) for t in (b.attn.proj.weight, b.attn.proj.bias, b.mlp.fc1.weight, b.mlp.fc1.bias, b.mlp.fc2.weight,
                                         b.mlp.fc2.bias, b.norm2.weight, b.norm2.bias))
            seq, b1f, pbf, b2f = hip.pack_block_seq(raw[0], raw[1], None, raw[2], raw[3], raw[4], raw[5], raw[6], raw[7], None, tdt)
            act_blocked = blocked and l > 0                       # the layout block l's QKV reads its rows in
            st = dict(raw=raw, wqf=wqf, bqf=bqf, xn_in=(hip.from_blocked16(xn) if act_blocked else xn)[:M].clone())
            if act_blocked:
                qkv = hip.gemm_blocked(xn, M, wqf, bqf, col_scale=S.QSCALE, scale_cols=384)
            else:
                qkv = hip.gemm(xn[:M], wqf, bqf, col_scale=S.QSCALE, scale_cols=384)
            hip.attention(qkv, n, N, heads, log2q=True, out_blocked=blocked, out=xn)          # the encoder reuses the xn buffer
            layout = 0
            if blocked:
                layout = hip.LAYOUT_ACT_BLOCKED | (hip.LAYOUT_X_IN_IMAGE if l > 0 else 0) | (hip.LAYOUT_X_OUT_IMAGE if l + 1 < enc.depth else 0)
            st.update(qkv=qkv, att=(hip.from_blocked16(xn) if blocked else xn)[:M].clone(),
                      x_in=(hip.from_image32(x) if layout & hip.LAYOUT_X_IN_IMAGE else x)[:M].clone())
            hip.block_fused_s(x[:M], xn[:M], seq, b1f, pbf, b2f, xn[:M] if l + 1 < enc.depth else None, layout=layout)
            st.update(x_out=(hip.from_image32(x) if layout & hip.LAYOUT_X_OUT_IMAGE else x)[:M].clone(),
                      xn_out=(hip.from_blocked16(xn) if blocked else xn)[:M].clone() if l + 1 < enc.depth else None)
            stages.append(st)
        cls = torch.empty(n, 384, device=dev)
        hip._check(hip.load().mst_layernorm(hip.ptr(x), N * 384, hip.ptr(f32(enc.norm.weight).contiguous()), hip.ptr(f32(enc.norm.bias).contiguous()),
                                            hip.ptr(cls), hip.F32, 384, n, 384, 1e-6, hip.stream_of(x)), "mst_layernorm")
        torch.cuda.synchronize()
    return cls, stages


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_fused_encode_replayed_op_by_op(hip, monkeypatch, dt):
    """A depth-3 ViT-S on 48 slices of 224 x 224: 12,336 tokens = 385.5 groups of 32 rows, the fused blocked plan with no environment
    variable set.  (1) The CLS rows of the chain rebuilt from the op wrappers are bit-equal to ``encode_slices``: the replay IS the
    encoder's chain.  (2) Every token row of the final x and of every layer's attention output is bit-equal to the same chain with
    everything row-major (predicted: the blocked attention epilogue and the blocked-A QKV GEMM change addresses only, see above;
    ``test_block_fused_single_role`` asserts the same of the block kernel's layouts).  (3) Every stage of the blocked chain is held to its
    op-level bar from the stage's own input: QKV at the bar of test_qkv_gemm_on_blocked_rows, attention at the bar of
    test_attention_encoder_contract, the block at the bars of tests/test_block_boundary_gpu.py.

    On MI355X, bf16 / fp16: (1) held / held.  (2) held / held, QKV rows included.  (3) QKV at most 0.936 / 0.777 of its bar, attention
    0.927 / 0.923, block x 3.95e-3 / 4.54e-4 of scale, xn 2.11e-2 / 2.45e-3."""
    for name in ("MST_FUSED_MIN_TOKENS", "MST_GEMM_WREG_MIN_M", "MST_PRUNE_LAST_BLOCK", "MST_CHUNK_SLICES", "MST_WS_BUDGET_MB"):
        monkeypatch.delenv(name, raising=False)
    n, N, heads = 48, 257, 6
    model = _model(dt)
    vol = synth.synth_volume((1, 1, n, 224, 224), 5).reshape(n, 224, 224).cuda()
    with torch.no_grad():
        emb, _, _ = model.encode_slices(vol)
    cls_b, blk = _chain(hip, model, vol, dt, True)
    assert torch.equal(cls_b, emb), "the replayed chain is not the encoder's"
    cls_r, row = _chain(hip, model, vol, dt, False)
    for l, (sb, sr) in enumerate(zip(blk, row)):
        assert torch.equal(sb["qkv"], sr["qkv"]), f"layer {l}: QKV differs between blocked and row-major rows"
        assert torch.equal(sb["att"], sr["att"]), f"layer {l}: attention output differs between the layouts"
        assert torch.equal(sb["x_out"], sr["x_out"]), f"layer {l}: x differs between the layouts"
    assert torch.equal(cls_b, cls_r)
    qs = float(torch.tensor(S.QSCALE, dtype=torch.float32))
    for l, st in enumerate(blk):
        ref = st["xn_in"].double() @ st["wqf"].double().t() + st["bqf"].double()
        ref[:, :384] *= qs
        r_qkv = S.worst_ratio(st["qkv"], ref, S.gemm_bar(ref, dt))
        aref, amag, _, _ = S.attn_ref2(st["qkv"], n, N, heads)               # on the device, in fp64
        r_att = S.worst_ratio(st["att"], aref, S.attn_bar(aref, amag, N, dt))
        xref, nref, scale = S.block_reference(st["x_in"], st["att"], st["raw"])
        e_x = float((st["x_out"].double() - xref).abs().max() / scale)
        e_n = float((st["xn_out"].double() - nref).abs().max()) if st["xn_out"] is not None else 0.0
        print(f"chain {dt} layer {l}: QKV {r_qkv:.3f} of its bar, attention {r_att:.3f} of its bar, block x {e_x:.2e} of scale "
              f"(bar {S.BLOCK_TOL[dt]:g}), xn {e_n:.2e} (bar {4 * S.BLOCK_TOL[dt]:g})")
        assert r_qkv <= 1.0 and r_att <= 1.0
        assert e_x < S.BLOCK_TOL[dt] and e_n < 4 * S.BLOCK_TOL[dt]
