#!/usr/bin/env python3
"""Device-side training augmentation (mst/augment.py) against its yardsticks, one JSON line per shape, appended to --out
(default profiles/augment.jsonl):

    augment_ms        TrainAugment(flip, random_rotate, noise)(batch): the host draws, the record upload, mst_volume_min and
                      mst_augment_volumes, per batch (HIP events around `reps` calls)
    kernel_ms         mst_augment_volumes alone on fixed records with every transform on; min_ms: mst_volume_min alone
    noise_only_ms / rotate_only_ms / flip_only_ms      the kernel with one transform on: where the time goes
    copy_ms           torch `copy_` of the same tensor into a second one, timed the same way in this script: the yardstick
    train_step_ms     the training step at that shape as tools/bench_train.py times it (fp16 linear products, flash attention, 16-bit storage: the fastest arm), unless --no-step

The arms alternate (a-b-a-b, the median of each), so that clock drift hits all alike."""
import argparse
import json
import sys
import warnings
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "new-vit_amd"), str(ROOT / "tools")]
warnings.simplefilter("ignore")
import torch
from mst import hip, synth
from mst.augment import TrainAugment


def ev(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def median(v):
    return sorted(v)[len(v) // 2]


def records(B, rotate, flip, noise, x):
    p = {"theta_deg": torch.full((B,), 33.0 if rotate else 0.0, dtype=torch.float64), "flip": torch.full((B, 3), bool(flip)),
         "sign": torch.full((B,), -1.0 if noise else 1.0, dtype=torch.float64), "noise_std": torch.full((B,), 0.2 if noise else 0.0, dtype=torch.float64)}
    rec = TrainAugment.record(p).cuda()
    return hip.volume_min(x, out=rec, column=hip.AUG_FILL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "augment.jsonl"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="fp32", choices=("fp32", "fp16", "bf16"))
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    dt = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}[a.dtype]
    lines = []
    for shape in ((2, 1, 32, 224, 224), (1, 1, 64, 518, 518)):
        B, _, D, H, W = shape
        batch = synth.synth_volume(shape, 3).cuda().to(dt)
        x = batch.view(B, D, H, W)
        dst = torch.empty_like(batch)
        aug = TrainAugment(flip=True, random_rotate=True, noise=True, generator=torch.Generator().manual_seed(0))
        rec_all, rec_noise = records(B, True, True, True, x), records(B, False, False, True, x)
        rec_rot, rec_flip = records(B, True, False, False, x), records(B, False, True, False, x)
        arms = {"augment_ms": lambda: aug(batch), "kernel_ms": lambda: hip.augment_volumes(x, rec_all, 1, 0),
                "min_ms": lambda: hip.volume_min(x, out=rec_all, column=hip.AUG_FILL),
                "noise_only_ms": lambda: hip.augment_volumes(x, rec_noise, 1, 0), "rotate_only_ms": lambda: hip.augment_volumes(x, rec_rot, 1, 0),
                "flip_only_ms": lambda: hip.augment_volumes(x, rec_flip, 1, 0), "copy_ms": lambda: dst.copy_(batch)}
        t = {k: [] for k in arms}
        for fn in arms.values():
            ev(fn, 3)                                        # warm-up of every arm
        for _ in range(a.rounds):
            for k, fn in arms.items():
                t[k].append(ev(fn, a.reps))
        res = {k: round(median(v), 4) for k, v in t.items()}
        nbytes = 2 * batch.numel() * batch.element_size()
        line = {"case": "TrainAugment(flip, random_rotate, noise) per batch, all transforms on", "shape": list(shape), "dtype": a.dtype, **res,
                "augment_over_copy": round(res["augment_ms"] / res["copy_ms"], 2), "kernel_over_copy": round(res["kernel_ms"] / res["copy_ms"], 2),
                "copy_GBps": round(nbytes / res["copy_ms"] / 1e6, 1), "kernel_GBps": round(nbytes / res["kernel_ms"] / 1e6, 1),
                "arms": "alternating", "rounds": a.rounds, "reps": a.reps, "all_augment_ms": [round(v, 4) for v in t["augment_ms"]],
                "all_copy_ms": [round(v, 4) for v in t["copy_ms"]]}
        if not a.no_step:
            import bench_train
            from mst.models import DinoV2ClassifierSlice
            m = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, train_precision="fp16", train_attention="flash", train_storage="16bit")
            m.load_state_dict(synth.synth_state_dict("s", 0))
            step = json.loads(bench_train.train_case("DinoV2ClassifierSlice training step (fp16 linear products, flash attention, 16bit storage, HIP backward)", m, shape,
                                                     n=3 if D >= 64 else 5))
            line["train_step_ms"] = step["train_step_ms"]
            line["augment_share_of_step"] = round(res["augment_ms"] / step["train_step_ms"], 4)
            del m
            torch.cuda.empty_cache()
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
