#!/usr/bin/env python3
"""SwiGLU on the 'g' encoder: what the fused GEMM epilogue buys, and what a forward costs.  A record, not a gate.

  A. the w12 product of one block at M = 21,920 token rows (16 x 1370), E = 1536, H = 4096, bf16:
       fused      mst_gemm(MST_EPI_BIAS_SWIGLU) on the row-paired image -> h [M, H]
       two-launch mst_gemm(MST_EPI_BIAS) -> x12 [M, 2H], then mst_swiglu_fwd16 -> h [M, H]
     alternating in one process after warm-up, device events around `--reps` calls each, `--rounds` rounds; both outputs are compared.
  B. the inference forward of a depth-4 'g' SwiGLU model (hub layout: LayerScale, 518 grid) at 1 x 16 x 518 x 518, bf16.

    python tools/bench_swiglu.py [--rounds 7] [--reps 20] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "new-vit_amd"))
import torch  # noqa: E402

from mst import hip  # noqa: E402


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(xs):
    return f"median {statistics.median(xs):.4f} ms, min {min(xs):.4f}, max {max(xs):.4f} over {len(xs)} rounds"


def epilogue(rounds, reps, say):
    M, E, H, dt = 16 * 1370, 1536, 4096, torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    a = torch.randn(M, E, device="cuda", generator=g).to(dt)
    w12 = torch.randn(2 * H, E, device="cuda", generator=g) / E ** 0.5
    b12 = torch.randn(2 * H, device="cuda", generator=g) * 0.1
    w12p, b12p, _ = hip.pack_swiglu(w12, b12, torch.zeros(E, H, device="cuda"), dt)
    w16 = w12.to(dt)
    h_fused = torch.empty(M, H, device="cuda", dtype=dt)
    x12 = torch.empty(M, 2 * H, device="cuda", dtype=dt)
    h_two = torch.empty(M, H, device="cuda", dtype=dt)
    lib, s = hip.load(), hip.stream_of(a)

    def fused():
        hip.gemm(a, w12p, b12p, epilogue=hip.EPI_BIAS_SWIGLU, out=h_fused)

    def two():
        hip.gemm(a, w16, b12, out=x12)
        hip._check(lib.mst_swiglu_fwd16(hip.ptr(x12), hip.ptr(h_two), hip.dt_of(x12), M, H, s), "mst_swiglu_fwd16")

    def plain():
        hip.gemm(a, w16, b12, out=x12)

    for fn in (fused, two):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    d = (h_fused.float() - h_two.float()).abs().max() / h_two.float().abs().max()
    say(f"A. w12 product, M = {M}, E = {E}, H = {H}, bf16; fused against two-launch output: max |d| / max |h| = {float(d):.3e} "
        "(the two-launch form rounds x12 to bf16 before the activation)")
    tf, tt, tp = [], [], []
    for _ in range(rounds):
        tf.append(timed(fused, reps))
        tt.append(timed(two, reps))
        tp.append(timed(plain, reps))
    flop = 2.0 * M * 2 * H * E
    say(f"   fused epilogue               : {spread(tf)}  ({flop / statistics.median(tf) / 1e9:.0f} TFLOP/s)")
    say(f"   bias GEMM + mst_swiglu_fwd16 : {spread(tt)}")
    say(f"   bias GEMM alone              : {spread(tp)}  ({flop / statistics.median(tp) / 1e9:.0f} TFLOP/s)")
    say(f"   fused / two-launch           : {statistics.median(tf) / statistics.median(tt):.3f} (medians); "
        f"slowest fused round {max(tf):.4f} ms against fastest two-launch round {min(tt):.4f} ms")


def forward(rounds, reps, say):
    from mst.models import DinoV2ClassifierSlice
    from mst.models.dino import _ViT
    depth = 4
    with torch.device("meta"):
        m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, model_size="g", ffn_layer="swiglufused", compute_dtype="bf16")
        m.encoder = _ViT(1536, depth, 24, img_size=518, layerscale=1.0, chunked=False, ffn_layer="swiglufused")
    m = m.to_empty(device="cuda").eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    with torch.no_grad():
        for k, p in m.named_parameters():                               # timing only: fan-in scaled weights, unit norms, small biases
            if p.dim() >= 2:
                p.copy_(torch.randn(p.shape, device="cuda", generator=g) / max(p.shape[-1], 1) ** 0.5)
            elif "norm" in k and k.endswith("weight") or k.endswith("gamma"):
                p.fill_(1.0)
            else:
                p.copy_(torch.randn(p.shape, device="cuda", generator=g) * 0.02)
    src = torch.randn(1, 1, 16, 518, 518, device="cuda", generator=g)
    with torch.no_grad():
        for _ in range(2):
            out = m(src)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        ts = [timed(lambda: m(src), max(1, reps // 4)) for _ in range(rounds)]
    say(f"B. depth-{depth} 'g' SwiGLU forward, 1 x 16 x 518 x 518, bf16 ({16 * 1370} token rows): {spread(ts)}; "
        f"{statistics.median(ts) / depth:.3f} ms per block (patch embedding and the across-slice stage included)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_swiglu needs an MI355X"
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"tools/bench_swiglu.py --rounds {args.rounds} --reps {args.reps} on {torch.cuda.get_device_name(0)}")
    epilogue(args.rounds, args.reps, say)
    forward(args.rounds, args.reps, say)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
