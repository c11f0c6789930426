#!/usr/bin/env python3
"""Timings that are NOT the headline, for the record: the training steps (forward + backward through the
HIP kernels + AdamW) of both model families, and the ViT-B forward on the unfused path.  One JSON line per case.
--deterministic: torch.use_deterministic_algorithms(True) for every case (the fixed-order reductions; DESIGN.md "Determinism");
--no-fill on top: torch.utils.deterministic.fill_uninitialized_memory = False, to tell torch's NaN fill from the kernels' cost.
--input-grad: the source-gradient timings (input_grad_cases, then resnet_input_grad_cases: --c3 adds the 1 x 128 x 512^2 shape, --out FILE
keeps the ResNet lines, --resnet-only skips the DinoV2ClassifierSlice cases).
--train-storage 16bit (beside --train-attention flash and a 16-bit precision): the encoder blocks' saved activations in 16 bits.  A comma
list (fp32,16bit,fp32) times those modes one after the other in this process: the repeated mode gives the spread the other is read against.
The same list drives the ResNet cases (train_storage of ResNetSliceTrans: --c3 for the configs[3] shape, --only-resnet for 2 x 32 x 224^2; add
--c3-only to --c3 to leave the smaller shape out).
--train-chunk-slices K[,K...] (DinoV2ClassifierSlice cases only; the ResNets have no such mode): train_chunk_slices of the model, one arm per
value in the given order in this process -- 0 is the plain step, the same-process baseline the others are read against.  --model-size g
(with it --steps N and --warmup W in place of the defaults) runs the arms on that encoder; --out FILE appends the DINOv2 lines to FILE."""
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


def resnet_input_grad_cases(c3, out_path):
    """--input-grad --resnet [--c3] [--out FILE]: gradients with respect to the source volume of ResNetSliceTrans(34), all in this process.
    Per shape and training mode (fp32, fp16, fp16 with 16-bit storage) the step with and without the source gradient, the two arms
    ALTERNATING (a-b-a-b, median of each) so that clock drift and allocator state hit both alike; a frozen eval-mode forward + backward
    (mst/train_resnet.py::_ResNetEvalFunction); then the stem's data gradient alone (mst_conv_dgrad_stem, HIP events) at 128 x 512^2, Cin 1,
    fp32: a `roofline` line against the algorithmic work (52.6 GFLOP, 2.1 GB of dz read, 134 MB written; fp32 MFMA peak 157 TF, HBM 8 TB/s)
    and the explicit forms it replaces -- mst_gemm_ex into a [rows, 64] matrix + mst_col2im_nhwc (atomics), and + the gather under the
    determinism flag.  `gate`: the new kernel is not slower than the gather form."""
    from mst import hip
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

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

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def median(v):
        return sorted(v)[len(v) // 2]
    shapes = [(2, 1, 32, 224, 224)] + ([(1, 1, 128, 512, 512)] if c3 else [])
    for shape in shapes:
        src = synth.synth_volume(shape, 3).cuda()
        tgt = torch.arange(shape[0]).cuda() % 2
        rounds = 3 if shape[2] >= 128 else 5
        for prec, st in (("fp32", "fp32"), ("fp16", "fp32"), ("fp16", "16bit")):
            m = ResNetSliceTrans(in_ch=1, out_ch=2, pretrained=False, model=34, train_precision=prec, train_storage=st)
            m.load_state_dict(synth.synth_resnet_state_dict(0, 34, 2), strict=True)
            m = m.cuda().train()

            def step(with_src):
                m.zero_grad(set_to_none=True)
                x = src.clone().requires_grad_(with_src)
                torch.nn.functional.cross_entropy(m(x), tgt).backward()
            step(False), step(True)                      # warm-up of both arms
            t = {False: [], True: []}
            for _ in range(rounds):
                for arm in (False, True):
                    t[arm].append(once(lambda: step(arm)))
            emit({"case": f"ResNetSliceTrans(resnet34) step, {prec} convolutions, {st} storage", "shape": list(shape), "arms": "alternating",
                  "rounds": rounds, "step_params_ms": round(median(t[False]), 2), "step_params_and_source_ms": round(median(t[True]), 2),
                  "all_params_ms": [round(v, 2) for v in t[False]], "all_params_and_source_ms": [round(v, 2) for v in t[True]]})
            del m
            torch.cuda.empty_cache()
        m = ResNetSliceTrans(in_ch=1, out_ch=2, pretrained=False, model=34)
        m.load_state_dict(synth.synth_resnet_state_dict(0, 34, 2), strict=True)
        m = m.cuda().eval().requires_grad_(False)

        def saliency():
            x = src.clone().requires_grad_(True)
            torch.autograd.grad(m(x)[:, 1].sum(), x)

        def fwd():
            with torch.no_grad():
                m(src)
        saliency(), fwd()
        ts, tf = [], []
        for _ in range(rounds):
            ts.append(once(saliency))
            tf.append(once(fwd))
        emit({"case": "ResNetSliceTrans(resnet34) frozen eval, fp32", "shape": list(shape), "arms": "alternating", "rounds": rounds,
              "frozen_source_only_fwd_bwd_ms": round(median(ts), 2), "no_grad_forward_ms": round(median(tf), 2)})
        del m
        torch.cuda.empty_cache()
    # the stem kernel alone, 128 x 512^2, one input channel, fp32
    n, H, W, Cout, K, kpad = 128, 512, 512, 64, 49, 64
    Ho = Wo = 256
    rows = n * Ho * Wo
    g = torch.Generator(device="cuda").manual_seed(0)
    dz = torch.randn(n, Ho, Wo, Cout, device="cuda", generator=g)
    wg = torch.zeros(Cout, kpad, device="cuda")
    wg[:, :K] = torch.randn(Cout, K, device="cuda", generator=g) * 0.1
    wk = wg[:, :K].contiguous()
    out = torch.empty(n, H, W, 1, device="cuda")
    col = torch.empty(rows, kpad, device="cuda")
    dx = torch.empty(n, H, W, 1, device="cuda")

    def explicit():
        hip.gemm_ex(dz.view(rows, Cout), wg, col, rows, kpad, Cout, sa=(Cout, 1), sb=(kpad, 1), sc=(kpad, 1))
        dx.zero_()
        hip.col2im_nhwc(col, dx, 7, 7, 2, 3)
    new_ms, atomic_ms = [], []
    for _ in range(3):                                   # arms alternating
        new_ms.append(ev(lambda: hip.conv_dgrad_stem(dz, wk, 7, 2, 3, H, W, 1, out=out)))
        atomic_ms.append(ev(explicit, 5))
    torch.use_deterministic_algorithms(True)
    gather_ms = []
    try:
        for _ in range(3):
            gather_ms.append(ev(explicit, 5))
    finally:
        torch.use_deterministic_algorithms("--deterministic" in sys.argv)
    ms = median(new_ms)
    fl = 2.0 * rows * Cout * K
    nbytes = 4.0 * (rows * Cout + n * H * W + Cout * K)
    tf, tbs = fl / ms / 1e9, nbytes / ms / 1e9
    emit({"case": f"mst_conv_dgrad_stem {n} x {H}x{W}, Cin=1, Cout={Cout}", "roofline": {
        "kernel": "stem_dgrad_kernel", "bound": "mfma" if fl / 157e12 > nbytes / 8e12 else "hbm", "achieved": round(tf, 1), "peak": 157.0,
        "unit": "TFLOP/s", "frac": round(tf / 157.0, 3), "achieved_GBps": round(tbs * 1e3, 1), "hbm_peak_TBps": 8.0, "frac_hbm": round(tbs / 8.0, 3),
        "flops_per_launch": fl, "bytes_per_launch": nbytes, "avg_launch_ms": round(ms, 4), "dtype": "fp32"}})
    emit({"case": "stem data gradient: mst_conv_dgrad_stem against mst_gemm_ex + mst_col2im_nhwc", "shape": [n, H, W, 1], "arms": "alternating",
          "conv_dgrad_stem_ms": [round(v, 3) for v in new_ms], "gemm_ex_col2im_atomic_ms": [round(v, 3) for v in atomic_ms],
          "gemm_ex_col2im_gather_ms": [round(v, 3) for v in gather_ms], "gate_not_slower_than_gather": bool(ms <= median(gather_ms)),
          "faster_than_atomic": bool(ms <= median(atomic_ms))})
    if out_path:
        Path(out_path).parent.mkdir(parents=True, exist_ok=True)
        Path(out_path).write_text("\n".join(lines) + "\n")
    if ms > median(gather_ms):
        sys.exit("gate: mst_conv_dgrad_stem is slower than the explicit gather form")


def train_case(name, model, shape, n=5, warm=2, extra=None):
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
    issued = []

    def steps_then_mark():                               # the host's share: how long issuing the n steps takes, the device still running
        for _ in range(n):
            step()
        issued.append(time.perf_counter())
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ms = timed(steps_then_mark, 1, 0) / n
    if extra is not None:
        extra = {**extra, "host_issue_ms": round((issued[0] - t0) / n * 1e3, 2)}
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    model.eval()
    ms_f = timed(fwd, n, warm)
    line = json.dumps({"case": name, "shape": list(shape), **(extra or {}), "train_step_ms": round(ms, 2), "eval_forward_ms": round(ms_f, 2),
                       "volumes_per_s_training": round(shape[0] / ms * 1e3, 2), "peak_GiB": round(peak, 2),
                       "deterministic": torch.are_deterministic_algorithms_enabled(),
                       "fill_uninitialized_memory": torch.utils.deterministic.fill_uninitialized_memory})
    print(line, flush=True)
    return line


def main():
    if "--deterministic" in sys.argv:                    # the fixed-order reductions of the training steps (mst.hip.deterministic)
        torch.use_deterministic_algorithms(True)
        if "--no-fill" in sys.argv:                      # attribution only: without torch's NaN fill of every torch.empty under the flag
            torch.utils.deterministic.fill_uninitialized_memory = False
    if "--input-grad" in sys.argv:
        if "--resnet-only" not in sys.argv:
            input_grad_cases()
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
        resnet_input_grad_cases("--c3" in sys.argv, out)
        return
    if "--rooflines" in sys.argv:
        backward_rooflines()
        attention_rooflines()
        return
    # --train-attention flash: the encoder blocks' attention without stored probabilities (16-bit precisions only; fp32 cases keep 'stored')
    attn = sys.argv[sys.argv.index("--train-attention") + 1] if "--train-attention" in sys.argv else "stored"
    # --train-storage 16bit | fp32,16bit,fp32: the blocks' saved activations (16-bit precisions with flash attention only; others keep 'fp32')
    storages = sys.argv[sys.argv.index("--train-storage") + 1].split(",") if "--train-storage" in sys.argv else ["fp32"]
    # --train-chunk-slices 0,16,8: the encoder recomputed per chunk of that many slices in the backward (0: its state kept), an arm per value
    chunked = "--train-chunk-slices" in sys.argv
    chunks = [int(v) for v in sys.argv[sys.argv.index("--train-chunk-slices") + 1].split(",")] if chunked else [0]
    size = sys.argv[sys.argv.index("--model-size") + 1] if "--model-size" in sys.argv else "s"
    steps = int(sys.argv[sys.argv.index("--steps") + 1]) if "--steps" in sys.argv else None
    warm = int(sys.argv[sys.argv.index("--warmup") + 1]) if "--warmup" in sys.argv else 2
    out = Path(sys.argv[sys.argv.index("--out") + 1]) if "--out" in sys.argv else None
    all_shapes = (("--only-dino-c1", (1, 1, 16, 224, 224)), ("--only-dino-2x32", (2, 1, 32, 224, 224)), ("--only-dino-518", (1, 1, 64, 518, 518)))
    dino_shapes = tuple(sh for flag, sh in all_shapes if flag in sys.argv) or tuple(sh for _, sh in all_shapes)    # several --only-dino-* add up
    for shape in (() if "--only-resnet" in sys.argv else dino_shapes):
        for prec in (("fp32", "bf16", "fp16") if "--mixed" in sys.argv else ("fp16",) if "--fp16" in sys.argv else ("bf16",) if "--bf16" in sys.argv else ("fp32",)):
            a = attn if prec != "fp32" else "stored"
            for st, k in ((st, k) for st in (storages if a == "flash" else ["fp32"]) for k in chunks):
                m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, model_size=size, train_precision=prec, train_attention=a,
                                          train_storage=st, train_chunk_slices=k)
                m.load_state_dict(synth.synth_state_dict(size, 0))
                line = train_case(f"DinoV2ClassifierSlice training step ({prec} linear products, {a} attention, {st} storage, HIP backward)"
                                  + (f", model_size {size}" if size != "s" else ""), m, shape, n=steps or (3 if shape[2] >= 64 else 5), warm=warm,
                                  extra={"model_size": size, "train_chunk_slices": k} if chunked else None)
                if out is not None:
                    out.parent.mkdir(parents=True, exist_ok=True)
                    with out.open("a") as f:
                        f.write(line + "\n")
                del m
                torch.cuda.empty_cache()
    if "--only-dino-c1" in sys.argv or "--only-dino-2x32" in sys.argv or "--only-dino-518" in sys.argv:
        return
    # the ResNet arms: --train-storage drives them too (the backbone's saved activations; 16-bit precisions only, fp32 keeps 'fp32'), one
    # model per arm in the given order in this process
    precs = ("fp32", "bf16", "fp16") if "--mixed" in sys.argv else ("fp16",) if "--fp16" in sys.argv else ("bf16",) if "--bf16" in sys.argv else ("fp32",)

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
