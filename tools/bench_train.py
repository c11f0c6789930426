#!/usr/bin/env python3
"""Timings that are NOT the headline, for the record: the training steps (forward + backward through the
HIP kernels + AdamW) of both model families, and the ViT-B forward on the unfused path.  One JSON line per case.
--deterministic: torch.use_deterministic_algorithms(True) for every case (the fixed-order reductions; DESIGN.md "Determinism");
--no-fill on top: torch.utils.deterministic.fill_uninitialized_memory = False, to tell torch's NaN fill from the kernels' cost.
--input-grad: the source-gradient timings (input_grad_cases).
--train-storage 16bit (beside --train-attention flash and a 16-bit precision): the encoder blocks' saved activations in 16 bits.  A comma
list (fp32,16bit,fp32) times those modes one after the other in this process: the repeated mode gives the spread the other is read against.
The same list drives the ResNet cases (train_storage of ResNetSliceTrans: --c3 for the configs[3] shape, --only-resnet for 2 x 32 x 224^2; add
--c3-only to --c3 to leave the smaller shape out)."""
import json
import sys
import time
import warnings
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "new-vit_amd")]
warnings.simplefilter("ignore")
import torch
from mst import synth
from mst.models import DinoV2ClassifierSlice, ResNetSliceTrans


def timed(fn, n, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def backward_rooflines():
    """`roofline` lines for the dominant BACKWARD kernels of the two training steps: algorithmic FLOPs of one launch
    / its HIP-event time against the dense MFMA peak of the operand type (bf16 / fp16 2.5 PF, fp32 MFMA 157 TF at the nominal clock)."""
    from mst import hip

    def ev(fn, n=20):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def line(case, kernel, flops, ms, peak_tf, dtype):
        tf = flops / ms / 1e9
        print(json.dumps({"case": case, "roofline": {"kernel": kernel, "bound": "mfma", "achieved": round(tf, 1), "peak": peak_tf, "unit": "TFLOP/s",
                                                     "frac": round(tf / peak_tf, 3), "flops_per_launch": flops, "avg_launch_ms": round(ms, 4), "dtype": dtype}}),
              flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    # (1) MST-DINOv2 mixed step, 2 x 32 x 224^2 = 16,448 tokens: d weight of fc1 (N 1536, K 384), the largest of the four per block
    M, N, K = 16448, 1536, 384
    dY, X = torch.randn(M, N, device="cuda", generator=g), torch.randn(M, K, device="cuda", generator=g)
    for dt, nm in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        d16, x16 = hip.cvt16(dY, dt), hip.cvt16(X, dt)
        sp, kc = 14, 1216
        at, xt = hip.cvt16(dY, dt, transpose=True, rows_pad=sp * kc), hip.cvt16(X, dt, transpose=True, rows_pad=sp * kc)
        line("DINOv2 mixed step 2x32x224^2: d weight fc1 = dY^T . X (transposed images, split-K 128x128x64 GEMM)", "gemm16_kernel (split-K)", 2.0 * M * N * K,
             ev(lambda: hip.gemm16_splitk(at, xt, sp)), 2500.0, nm)
        line("same product through the transposing-read kernel", "wgrad16_kernel", 2.0 * M * N * K, ev(lambda: hip.conv_wgrad(d16, x16.view(M, 1, 1, K), 1, 1, 0)), 2500.0, nm)
        w16 = hip.cvt16(torch.randn(N, K, device="cuda", generator=g), dt, transpose=True)
        line("DINOv2 mixed step: d input of fc1 = dY . W", "gemm16 family", 2.0 * M * N * K, ev(lambda: hip.gemm(d16, w16, None, out_dtype=torch.float32)), 2500.0, nm)
    dW = torch.empty(N, K, device="cuda")
    line("DINOv2 fp32 step: d weight fc1 (strided fp32 MFMA GEMM, 16 slabs)", "gemm_ex_kernel<2,2>", 2.0 * M * N * K,
         ev(lambda: hip.gemm_ex(dY, X, torch.empty(16, N * K, device="cuda"), N, K, M // 16, sa=(1, N), sb=(K, 1), sc=(K, 1), nb=(16, 1), ba=(M // 16 * N, 0),
                                bb=(M // 16 * K, 0), bc=(N * K, 0))), 157.0, "fp32")
    # (2) ResNet-34 step at the configs[3] per-GPU shape (128 images of 512^2): the layer-1 3x3 convolution (64 -> 64 channels at 128 x 128)
    n, H, C, k = 128, 128, 64, 3
    x = torch.randn(n, H, H, C, device="cuda", generator=g)
    dz = torch.randn(n * H * H, C, device="cuda", generator=g)
    fl = 2.0 * n * H * H * C * C * k * k
    line("ResNet-34 fp32 step 128x512^2: d weight of a layer-1 convolution (implicit GEMM)", "wgrad32_kernel", fl, ev(lambda: hip.conv_wgrad(dz, x, k, 1, 1), 5), 157.0, "fp32")
    x16, dz16 = hip.cvt16(x.view(-1, C), torch.bfloat16).view(x.shape), hip.cvt16(dz, torch.bfloat16)
    line("ResNet-34 mixed step: the same d weight on bf16 operands (transposing LDS reads)", "wgrad16_kernel", fl, ev(lambda: hip.conv_wgrad(dz16, x16, k, 1, 1), 5), 2500.0, "bf16")
    wt = torch.randn(C, k * k * C, device="cuda", generator=g).to(torch.bfloat16)
    line("ResNet-34 mixed step: d input of that convolution (implicit GEMM, gathered LDS-DMA)", "conv16_kernel", fl, ev(lambda: hip.conv_dgrad(dz16.view(n, H, H, C), wt, k, 1, 1, H, H), 5), 2500.0, "bf16")


def attention_rooflines():
    """`roofline` lines for the memory-efficient training attention (csrc/k_attn16_train.hip) at the encoder shapes of 2 x 32 x 224^2 and
    64 x 518^2 (64 sequences x 6 heads): algorithmic FLOPs only (forward 4 n h N^2 64, backward 8 n h N^2 64 -- the recomputed S and dP are
    not credited) against the dense 16-bit MFMA peak."""
    from mst import hip

    def ev(fn, n=10):
        for _ in range(2):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n
    g = torch.Generator(device="cuda").manual_seed(0)
    for N in (257, 1370):
        n, h = 64, 6
        for dt, nm in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
            x = torch.randn(n * N, 3, h, 64, device="cuda", generator=g)
            x[:, 0] *= 0.125
            qkv = x.view(n * N, 3 * h * 64).to(dt)
            out, lse = hip.attention_train_fwd(qkv, n, N, h)
            dout = torch.randn_like(out)
            dqkv = torch.empty(n * N, 3 * h * 64, device="cuda")
            for kernel, fl, fn in (("attn_train_fwd_kernel", 4.0 * n * h * N * N * 64, lambda: hip.attention_train_fwd(qkv, n, N, h)),
                                   ("attn_train_pre + dkv + dq kernels", 8.0 * n * h * N * N * 64,
                                    lambda: hip.attention_train_bwd(qkv, out, dout, lse, n, N, h, 0.125, dqkv=dqkv))):
                ms = ev(fn)
                tf = fl / ms / 1e9
                print(json.dumps({"case": f"DINOv2 flash training attention {n} x {h} heads x N={N}", "roofline": {
                    "kernel": kernel, "bound": "mfma", "achieved": round(tf, 1), "peak": 2500.0, "unit": "TFLOP/s", "frac": round(tf / 2500.0, 3),
                    "flops_per_launch": fl, "avg_launch_ms": round(ms, 4), "dtype": nm}}), flush=True)


def input_grad_cases():
    """--input-grad: gradients with respect to the source volume (mst_patch_embed_dgrad + the encoder's d x chain).  Per case one JSON line
    with the full step (parameters and source), the same step without the source gradient, and a frozen-parameter source-only backward
    (saliency); then a `roofline` line for mst_patch_embed_dgrad alone (HIP events) against the fp32 MFMA peak (157 TF) and HBM (8 TB/s)."""
    from mst import hip

    def ev(fn, n=20):
        for _ in range(3):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n
    for shape, prec, attn in (((2, 1, 32, 224, 224), "fp16", "flash"), ((1, 1, 64, 518, 518), "fp16", "flash")):
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, train_precision=prec, train_attention=attn)
        m.load_state_dict(synth.synth_state_dict("s", 0))
        m = m.cuda().train()
        src = synth.synth_volume(shape, 3).cuda()
        tgt = torch.arange(shape[0]).cuda() % 2
        reps = 3 if shape[2] >= 64 else 5

        def step(with_src):
            m.zero_grad(set_to_none=True)
            x = src.clone().requires_grad_(with_src)
            torch.nn.functional.cross_entropy(m(x), tgt).backward()
        ms_params = timed(lambda: step(False), reps)
        ms_full = timed(lambda: step(True), reps)
        m.requires_grad_(False)
        m.eval()

        def saliency():
            x = src.clone().requires_grad_(True)
            torch.autograd.grad(m(x)[:, 1].sum(), x)
        ms_src = timed(saliency, reps)
        print(json.dumps({"case": f"DinoV2ClassifierSlice input gradient ({prec} linear products, {attn} attention)", "shape": list(shape),
                          "step_params_ms": round(ms_params, 2), "step_params_and_source_ms": round(ms_full, 2),
                          "frozen_source_only_fwd_bwd_ms": round(ms_src, 2)}), flush=True)
        del m
        torch.cuda.empty_cache()
        # the kernel alone at this shape: ViT-S/14 (E 384) and, for scale, ViT-L/14 (E 1024)
        B, C, D, H, W = shape
        n, Np = B * C * D, (H // 14) * (W // 14)
        for E in (384, 1024):
            g = torch.Generator(device="cuda").manual_seed(0)
            dx = torch.randn(n * (1 + Np), E, device="cuda", generator=g)
            wsum = torch.randn(E, 224, device="cuda", generator=g)
            out = torch.empty(n, H, W, device="cuda")
            ms = ev(lambda: hip.patch_embed_dgrad(dx, wsum, n, H, W, tokens=1 + Np, first=1, out=out))
            fl = 2.0 * n * Np * E * 196
            nbytes = 4.0 * (n * Np * E + n * H * W + E * 224)
            tf, tbs = fl / ms / 1e9, nbytes / ms / 1e9
            print(json.dumps({"case": f"mst_patch_embed_dgrad {n} x {H}x{W}, E={E}", "roofline": {
                "kernel": "patch_dgrad_kernel", "bound": "mfma" if fl / 157e12 > nbytes / 8e12 else "hbm", "achieved": round(tf, 1), "peak": 157.0,
                "unit": "TFLOP/s", "frac": round(tf / 157.0, 3), "achieved_TBps": round(tbs, 2), "hbm_peak_TBps": 8.0,
                "frac_hbm": round(tbs / 8.0, 3), "flops_per_launch": fl, "bytes_per_launch": nbytes, "avg_launch_ms": round(ms, 4),
                "dtype": "fp32"}}), flush=True)


def train_case(name, model, shape, n=5):
    model = model.cuda().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    src = synth.synth_volume(shape, 3).cuda()
    tgt = torch.arange(shape[0]).cuda() % 2

    def step():
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.cross_entropy(model(src), tgt)
        loss.backward()
        opt.step()

    def fwd():
        with torch.no_grad():
            model(src)
    torch.cuda.reset_peak_memory_stats()
    ms = timed(step, n)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    model.eval()
    ms_f = timed(fwd, n)
    print(json.dumps({"case": name, "shape": list(shape), "train_step_ms": round(ms, 2), "eval_forward_ms": round(ms_f, 2),
                      "volumes_per_s_training": round(shape[0] / ms * 1e3, 2), "peak_GiB": round(peak, 2),
                      "deterministic": torch.are_deterministic_algorithms_enabled(),
                      "fill_uninitialized_memory": torch.utils.deterministic.fill_uninitialized_memory}), flush=True)


def main():
    if "--deterministic" in sys.argv:                    # the fixed-order reductions of the training steps (mst.hip.deterministic)
        torch.use_deterministic_algorithms(True)
        if "--no-fill" in sys.argv:                      # attribution only: without torch's NaN fill of every torch.empty under the flag
            torch.utils.deterministic.fill_uninitialized_memory = False
    if "--input-grad" in sys.argv:
        input_grad_cases()
        return
    if "--rooflines" in sys.argv:
        backward_rooflines()
        attention_rooflines()
        return
    # --train-attention flash: the encoder blocks' attention without stored probabilities (16-bit precisions only; fp32 cases keep 'stored')
    attn = sys.argv[sys.argv.index("--train-attention") + 1] if "--train-attention" in sys.argv else "stored"
    # --train-storage 16bit | fp32,16bit,fp32: the blocks' saved activations (16-bit precisions with flash attention only; others keep 'fp32')
    storages = sys.argv[sys.argv.index("--train-storage") + 1].split(",") if "--train-storage" in sys.argv else ["fp32"]
    all_shapes = (("--only-dino-c1", (1, 1, 16, 224, 224)), ("--only-dino-2x32", (2, 1, 32, 224, 224)), ("--only-dino-518", (1, 1, 64, 518, 518)))
    dino_shapes = tuple(sh for flag, sh in all_shapes if flag in sys.argv) or tuple(sh for _, sh in all_shapes)    # several --only-dino-* add up
    for shape in (() if "--only-resnet" in sys.argv else dino_shapes):
        for prec in (("fp32", "bf16", "fp16") if "--mixed" in sys.argv else ("fp16",) if "--fp16" in sys.argv else ("fp32",)):
            a = attn if prec != "fp32" else "stored"
            for st in (storages if a == "flash" else ["fp32"]):
                m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, train_precision=prec, train_attention=a, train_storage=st)
                m.load_state_dict(synth.synth_state_dict("s", 0))
                train_case(f"DinoV2ClassifierSlice training step ({prec} linear products, {a} attention, {st} storage, HIP backward)", m, shape,
                           n=3 if shape[2] >= 64 else 5)
                del m
                torch.cuda.empty_cache()
    if "--only-dino-c1" in sys.argv or "--only-dino-2x32" in sys.argv or "--only-dino-518" in sys.argv:
        return
    # the ResNet arms: --train-storage drives them too (the backbone's saved activations; 16-bit precisions only, fp32 keeps 'fp32'), one
    # model per arm in the given order in this process
    precs = ("fp32", "bf16", "fp16") if "--mixed" in sys.argv else ("fp16",) if "--fp16" in sys.argv else ("fp32",)

    def resnet_arms(case, shape, precs, n):
        for prec in precs:
            for st in (storages if prec != "fp32" else ["fp32"]):
                m = ResNetSliceTrans(in_ch=1, out_ch=2, pretrained=False, model=34, train_precision=prec, train_storage=st)
                m.load_state_dict(synth.synth_resnet_state_dict(0, 34, 2), strict=True)
                train_case(case(prec) + (f", {st} storage" if "--train-storage" in sys.argv else ""), m, shape, n=n)
                del m
                torch.cuda.empty_cache()
    if "--c3-only" not in sys.argv:
        # the fp32 case as before; with --train-storage the 16-bit arms of --fp16 / --mixed instead
        resnet_arms(lambda prec: "ResNetSliceTrans(resnet34) training step (fp32 HIP backward)" if prec == "fp32" else
                    f"ResNetSliceTrans(resnet34) training step ({prec} convolutions)", (2, 1, 32, 224, 224),
                    precs if "--train-storage" in sys.argv else ("fp32",), 5)
    if "--c3" in sys.argv:                               # BASELINE configs[3] per-GPU shape: one LIDC-shaped 128 x 512 x 512 volume
        resnet_arms(lambda prec: f"ResNetSliceTrans(resnet34) training step ({prec} convolutions), BASELINE configs[3] shape",
                    (1, 1, 128, 512, 512), precs, 3)
        return
    if "--only-resnet" in sys.argv:
        return
    # ViT-B forward at the bench batch (unfused path: LayerNorm + four GEMMs + attention per block)
    m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, model_size="b", compute_dtype="bf16")
    m.load_state_dict(synth.synth_state_dict("b", 0))
    m = m.cuda().eval()
    src = torch.randn(4, 1, 64, 518, 518, device="cuda", dtype=torch.bfloat16)

    def fwd():
        with torch.no_grad():
            m(src)
    ms = timed(fwd, 5)
    N, E, depth = 1370, 768, 12
    fl = 256 * (2 * 1369 * E * 588 + depth * (24 * N * E * E + 4 * N * N * E))
    print(json.dumps({"case": "ViT-B/14 forward, 4 x 64 x 518^2 bf16 (unfused blocks)", "ms": round(ms, 2), "volumes_per_s": round(4 / ms * 1e3, 2),
                      "tflops": round(fl / ms / 1e9, 1)}), flush=True)


if __name__ == "__main__":
    main()
