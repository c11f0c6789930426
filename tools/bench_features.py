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

--grad: what a TRAINING call of the API costs (``encoder_grad=True``).  forward_features on [n, 3, H, W], a loss over the patch tokens,
``backward()`` with every encoder parameter and x asking for a gradient: forward + backward ms (device events, median of --rounds rounds of
--reps calls) and the peak allocated bytes of one call above what is allocated before it, at 8 x 3 x 224^2 and 2 x 3 x 518^2, in fp32 and
in bf16 / flash / 16bit; one JSON line each into profiles/encoder_features_grad.jsonl.  --classifier FILE: JSON lines of the classifier's
training step at the same slice count and size (1 x 1 x 8 x 224^2, 1 x 1 x 2 x 518^2), taken with tools/bench_train.py's `train_case` on
the parent commit; the line whose "shape" and "mode" match goes beside each record as "classifier_step".  No time is promised and
nothing is gated on one: the lines are the record.

    python tools/bench_features.py --grad [--classifier FILE] [--out profiles/encoder_features_grad.jsonl]
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


GRAD_SHAPES = ((8, 3, 224, 224), (2, 3, 518, 518))
GRAD_MODES = (("fp32", {}), ("bf16/flash/16bit", dict(train_precision="bf16", train_attention="flash", train_storage="16bit")))


def grad_lines(args):
    beside = [json.loads(ln) for ln in Path(args.classifier).read_text().splitlines() if ln.strip()] if args.classifier else []
    lines = []
    for mode, kw in GRAD_MODES:
        model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype="fp32", encoder_grad=True, **kw)
        model.load_state_dict(synth.synth_state_dict("s", 0), strict=True)
        model = model.cuda().train()
        enc = model.encoder
        for shape in GRAD_SHAPES:
            n, _, H, W = shape
            x = torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(n)).requires_grad_()

            def call():
                enc.forward_features(x)["x_norm_patchtokens"].square().mean().backward()
            for _ in range(2):
                call()
            model.zero_grad(set_to_none=True)
            x.grad = None
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            call()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            t = [timed(call, args.reps) for _ in range(args.rounds)]
            rec = dict(bench="encoder_features_grad", device=torch.cuda.get_device_name(0), mode=mode, shape=list(shape),
                       tokens=n * (1 + (H // 14) * (W // 14)), call="forward_features -> patch-token loss -> backward (all encoder parameters, x)",
                       fwd_bwd_ms_median=round(statistics.median(t), 3), fwd_bwd_ms_min=round(min(t), 3), fwd_bwd_ms_max=round(max(t), 3),
                       rounds=args.rounds, reps=args.reps, peak_allocated_bytes_above_start=int(peak),
                       classifier_step=next((b for b in beside if b.get("shape") == [1, 1, n, H, W] and b.get("mode") == mode), None))
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
            del x
            model.zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mode", default="bf16")
    ap.add_argument("--out", default=None)
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--classifier", default=None)
    args = ap.parse_args()
    args.out = args.out or str(ROOT / "profiles" / ("encoder_features_grad.jsonl" if args.grad else "encoder_features.jsonl"))
    assert torch.cuda.is_available(), "bench_features needs an MI355X"
    if args.grad:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(grad_lines(args)) + "\n")
        return
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
