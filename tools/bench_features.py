#!/usr/bin/env python3
"""What the encoder API costs beside the class-token-only encoder.  A record, not a gate.

Arms, alternating in one process after warm-up (device events around `--reps` calls each, `--rounds` rounds), on the same grey slices:
    encode_slices              the unchanged hot path: normalised class tokens only
    forward_features           + x_prenorm of every token (one tap) and encoder.norm of every row
    get_intermediate_layers4   get_intermediate_layers(n=4): four normalised taps
    forward_features_rgb       forward_features on [n, 3, H, W]: the three-channel patch embedding (K = 588) instead of the folded one
at 4 x 64 x 518 x 518 (350,720 tokens) and 1 x 32 x 224 x 224 (8,224 tokens), bf16, seed-0 synthetic ViT-S weights.
One JSON line per shape and arm; `bytes_out` is what the arm returns (fp32), computed from the shapes.

    python tools/bench_features.py [--rounds 7] [--reps 5] [--out profiles/encoder_features.jsonl]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "new-vit_amd"))
import torch  # noqa: E402

from mst import synth  # noqa: E402
from mst.models import DinoV2ClassifierSlice  # noqa: E402

SHAPES = ((4, 64, 518, 518), (1, 32, 224, 224))


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "encoder_features.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_features needs an MI355X"
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=args.mode)
    model.load_state_dict(synth.synth_state_dict("s", 0), strict=True)
    model = model.cuda().eval()
    enc = model.encoder
    E = enc.embed_dim
    lines = []
    with torch.no_grad():
        for B, D, H, W in SHAPES:
            n, N = B * D, 1 + (H // 14) * (W // 14)
            g = torch.Generator(device="cuda").manual_seed(B * D)
            grey = torch.randn(n, 1, H, W, device="cuda", generator=g)
            rgb = torch.randn(n, 3, H, W, device="cuda", generator=g)
            slices = grey[:, 0]
            arms = {
                "encode_slices": (lambda: model.encode_slices(slices), n * E * 4),
                "forward_features": (lambda: enc.forward_features(grey), 2 * n * N * E * 4),
                "get_intermediate_layers4": (lambda: enc.get_intermediate_layers(grey, n=4), 4 * n * N * E * 4),
                "forward_features_rgb": (lambda: enc.forward_features(rgb), 2 * n * N * E * 4),
            }
            for fn, _ in arms.values():                  # warm-up: LDS attributes, workspaces, the position grid, the RGB kernel image
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            assert torch.equal(enc.forward_features(grey)["x_norm_clstoken"], model.encode_slices(slices)[0])
            times = {k: [] for k in arms}
            for _ in range(args.rounds):
                for k, (fn, _) in arms.items():
                    times[k].append(timed(fn, args.reps))
            base = statistics.median(times["encode_slices"])
            for k, (_, nbytes) in arms.items():
                t = times[k]
                rec = dict(bench="encoder_features", device=torch.cuda.get_device_name(0), mode=args.mode, shape=[B, D, H, W], tokens=n * N,
                           arm=k, ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                           rounds=args.rounds, reps=args.reps, bytes_out=nbytes,
                           over_encode_slices_ms=round(statistics.median(t) - base, 4))
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
            del grey, rgb, slices, arms
            torch.cuda.empty_cache()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
