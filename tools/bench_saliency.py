#!/usr/bin/env python3
"""`--get_attention` / `--use_tta` path of scripts/main_predict.py through mst.saliency.run_pred.

Without options: the c3 shape (1 x 64 x 518^2, fp32 parity mode and bf16), run_pred with and without TTA, and the up-sampling kernel
alone against its HBM roofline (68.7 MB written once).

    --tta loop,folded   test-time augmentation only: one JSON line per mode and shape with the ms per volume of
                        run_pred(use_tta=True), without and with save_attn (median of --repeats timed windows, every window listed).
                        "loop" is called without the `tta` keyword, so that with --package-root the same tool times another checkout
                        of this package (one from before the folded mode, say) in the same session.
    --shapes            BxDxHxW[,...]; H and W multiples of 14 (default 1x32x224x224,1x64x518x518: 518 is what '512^2' becomes)
    --dtype             compute dtype of the model (default bf16); the volume is fp32, as the datasets emit it
"""
import argparse, json, statistics, sys, time
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--tta", default=None, help="comma-separated TTA modes to time: loop, folded")
ap.add_argument("--shapes", default="1x32x224x224,1x64x518x518")
ap.add_argument("--dtype", default="bf16")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--window-s", type=float, default=0.5, help="least duration of one timed window")
ap.add_argument("--package-root", default=None, help="checkout whose new-vit_amd/mst is measured (default: this one)")
ap.add_argument("--label", default=None, help="copied into every JSON line")
args = ap.parse_args()

ROOT = Path(args.package_root).resolve() if args.package_root else Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "new-vit_amd")]
import torch
from mst import hip, synth
from mst.models import DinoV2ClassifierSlice
from mst.saliency import run_pred


def build(mode):
    model = DinoV2ClassifierSlice(in_ch=1, out_ch=2, pretrained=False, compute_dtype=mode)
    model.load_state_dict(synth.synth_state_dict("s", 0))
    return model.cuda().eval()


def timed_windows(fn, repeats, window_s):
    """ms per call of fn over `repeats` windows, each of enough calls to last window_s and ended by a device synchronise."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    calls = max(3, int(window_s / max(time.perf_counter() - t0, 1e-4)) + 1)
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / calls * 1e3)
    return calls, out


def bench_tta():
    modes = [m.strip() for m in args.tta.split(",") if m.strip()]
    for m in modes:
        if m not in ("loop", "folded"):
            sys.exit(f"--tta: unknown mode {m!r} (loop, folded)")
    model = build(args.dtype)
    for shape in args.shapes.split(","):
        B, D, H, W = (int(v) for v in shape.split("x"))
        src = torch.randn(B, 1, D, H, W, device="cuda")
        for m in modes:
            kw = {} if m == "loop" else {"tta": m}
            line = {"bench": "run_pred_tta", "label": args.label, "package": str(ROOT.name), "tta": m, "shape": [B, 1, D, H, W],
                    "dtype": args.dtype, "input_dtype": "fp32", "repeats": args.repeats}
            for save_attn in (False, True):
                if save_attn and B != 1:
                    continue
                calls, ms = timed_windows(lambda: run_pred(model, {"source": src}, save_attn=save_attn, use_tta=True, **kw),
                                          args.repeats, args.window_s)
                key = "save_attn" if save_attn else "pred_only"
                line[key] = {"ms_per_volume": round(statistics.median(ms) / B, 3), "min": round(min(ms) / B, 3),
                             "max": round(max(ms) / B, 3), "runs_ms": [round(v / B, 3) for v in ms], "calls_per_run": calls}
            print(json.dumps(line), flush=True)


def bench_c3():
    low = torch.rand(64, 37, 37, device="cuda")
    for _ in range(3):
        out = hip.saliency_upsample(low, (64, 518, 518), 0.125)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        out = hip.saliency_upsample(low, (64, 518, 518), 0.125)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 50
    print({"upsample_ms": round(ms, 4), "GB_per_s_written": round(out.numel() * 4 / ms / 1e6, 1), "hbm_peak_GB_per_s": 8000})

    src = torch.randn(1, 1, 64, 518, 518, device="cuda")
    for mode in ("bf16", "fp32"):
        model = build(mode)
        for tta in (False, True):
            run_pred(model, {"source": src}, save_attn=True, use_tta=tta)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 5
            for _ in range(n):
                run_pred(model, {"source": src}, save_attn=True, use_tta=tta)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            print({"mode": mode, "use_tta": tta, "ms_per_volume": round(dt * 1e3, 2), "volumes_per_s": round(1 / dt, 2)})


if __name__ == "__main__":
    if args.tta is not None:
        bench_tta()
    else:
        bench_c3()
