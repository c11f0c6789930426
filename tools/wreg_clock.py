#!/usr/bin/env python3
"""Steady-state time of the QKV GEMM (M = 350,720): 2 s of back-to-back launches first, so that the power-limited clock has
settled, then 20 timed launches."""
import sys, time
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "new-vit_amd"))
import torch
from mst import hip
M, N, K = 350720, 1152, 384
torch.manual_seed(0)
a = torch.randn(M, K, device="cuda").bfloat16()
w = (torch.randn(N, K, device="cuda") / K ** 0.5).bfloat16()
b = torch.randn(N, device="cuda")
out = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
t0 = time.time()
while time.time() - t0 < 2.0:
    for _ in range(50):
        hip.gemm(a, w, b, epilogue=0, out=out)
    torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    hip.gemm(a, w, b, epilogue=0, out=out)
e1.record()
torch.cuda.synchronize()
print({"ms": round(e0.elapsed_time(e1) / 20, 4)})
