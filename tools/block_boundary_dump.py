#!/usr/bin/env python3
"""Dump block_fused_s outputs (x and xn) for bf16 / fp16, layouts 0 and 7, at the bench's M = 350,720 rows as .npy files:
    MST_HIP_LIB=<library> python tools/block_boundary_dump.py DIR
Run once per library in a fresh process and compare the directories with np.array_equal (profiles/block_boundary_bit_equality_*.md)."""
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "new-vit_amd"))
import numpy as np
import torch
from mst import hip
out = Path(sys.argv[1]); out.mkdir(parents=True, exist_ok=True)
M, E, H = 350720, 384, 1536
for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
    torch.manual_seed(0)
    g = lambda *s: torch.randn(*s, device="cuda")
    x0 = g(M, E); att = g(M, E).to(dt)
    seq, b1f, pbf, b2f = hip.pack_block_seq(g(E, E) / E ** .5, g(E) * .1, None, g(H, E) / E ** .5, g(H) * .1, g(E, H) / H ** .5, g(E) * .1,
                                            torch.ones(E, device="cuda"), torch.zeros(E, device="cuda"), None, dt)
    for layout in (0, 7):
        x = hip.to_image32(x0) if layout else x0.clone()
        a = hip.to_blocked16(att) if layout else att.clone()
        xn = torch.empty(M, E, device="cuda", dtype=dt)
        hip.block_fused_s(x, a, seq, b1f, pbf, b2f, xn, layout=layout)
        torch.cuda.synchronize()
        np.save(out / f"{name}_layout{layout}_x.npy", x.cpu().numpy())
        np.save(out / f"{name}_layout{layout}_xn.npy", xn.view(torch.int16).cpu().numpy())
        print(name, layout, "dumped")
