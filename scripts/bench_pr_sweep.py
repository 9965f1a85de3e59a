"""Time estimate_metrics.pr_sweep (tolerance-matched precision / recall counts over the threshold sweep, csrc/pr_sweep.hip) next to
iou_sweep and surface_distance_sweep on the same tensors in the same process, and evaluate_dataset with and without pr_tolerance.

    python scripts/bench_pr_sweep.py                      # writes profiles/pr_sweep_bench.json and prints it as one JSON line

  sweeps   8 maps of 1792^2: sparse synthetic crack masks (csbsr_amd/data/synthetic.py) and model-like maps (the mask two or three pixels off
           centre, blurred, plus faint noise).  Device events around ``reps`` calls after a warm-up (500 by default: a window of a tenth
           of a second; surface_distance_sweep, a second per call, 20); five such windows per call, the median reported with the spread
           (max / min - 1).  A call is the Python call: workspace allocation, zeroing and both launches.  pr_sweep reads 8 bytes per pixel
           (pred and mask once): achieved bytes / s from that.  Kernel times: the same leg under ``rocprofv3 --kernel-trace --stats``
           (--reps 50 --sd-reps 1), profiles/pr_sweep_kernel_stats.csv.
  dataset  evaluate_dataset without saving over 48 synthetic 448^2 images, config-2 model (deterministic fill), batch 12: one warm-up pass
           each, then five whole passes with pr_tolerance = 2 and five without, alternating."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def windows(fn, reps, warmup, n_windows=5):
    """event ms per call of fn(): ``n_windows`` windows of ``reps`` calls after ``warmup`` calls -> (median, spread, all)"""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(n_windows):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return float(np.median(ms)), max(ms) / min(ms) - 1, ms


def crack_maps(n, size, seed=21):
    from csbsr_amd.data.synthetic import crack_masks
    mask = crack_masks(n, size, size, torch.Generator().manual_seed(seed)).to(DEV)
    shifted = torch.roll(mask, (3, -2), (2, 3))
    prob = torch.nn.functional.avg_pool2d(shifted, 7, 1, 3)
    noise = torch.randn(prob.shape, generator=torch.Generator(device=DEV).manual_seed(seed + 1), device=DEV)
    return (prob + 0.02 * noise).clamp(0, 1).contiguous(), mask.contiguous()


def leg_sweeps(a):
    from csbsr_amd.inference import THRESHOLDS
    from csbsr_amd.utils.estimate_metrics import iou_sweep, pr_sweep, surface_distance_sweep
    prob, mask = crack_maps(a.maps, a.size)
    npix = prob.numel()
    out = {"maps": a.maps, "size": a.size, "thresholds": len(THRESHOLDS), "reps": a.reps, "warmup": a.warmup,
           "gt_fraction": round(float((mask > 0.5).float().mean()), 5), "level_gt0_fraction": round(float((prob > 0.01).float().mean()), 5)}
    c0 = pr_sweep(prob, mask, THRESHOLDS, 0).cpu().numpy().astype(np.int64)
    c2 = pr_sweep(prob, mask, THRESHOLDS, 2).cpu().numpy().astype(np.int64)
    out["repeat_identical"] = bool(np.array_equal(c2, pr_sweep(prob, mask, THRESHOLDS, 2).cpu().numpy()))
    out["recall_at_0.50_tolerance_0_vs_2"] = [round(float(c[:, 2, 49].sum() / c[:, 3, 49].sum()), 4) for c in (c0, c2)]
    for tol in (0, 2, 5):
        med, spread, _ = windows(lambda: pr_sweep(prob, mask, THRESHOLDS, tol), a.reps, a.warmup)
        out[f"pr_sweep_tol{tol}_ms"] = round(med, 4)
        out[f"pr_sweep_tol{tol}_spread"] = round(spread, 4)
        out[f"pr_sweep_tol{tol}_GBps"] = round(8 * npix / (med * 1e-3) / 1e9, 1)
    med, spread, _ = windows(lambda: iou_sweep(prob, mask, THRESHOLDS), a.reps, a.warmup)
    out.update(iou_sweep_ms=round(med, 4), iou_sweep_spread=round(spread, 4), iou_sweep_GBps=round(8 * npix / (med * 1e-3) / 1e9, 1))
    med, spread, _ = windows(lambda: surface_distance_sweep(prob, mask, THRESHOLDS), a.sd_reps, 1, n_windows=1)
    out.update(surface_distance_sweep_ms=round(med, 2), surface_distance_reps=a.sd_reps)
    out["pr_tol2_over_iou_sweep"] = round(out["pr_sweep_tol2_ms"] / out["iou_sweep_ms"], 2)
    out["surface_distance_over_pr_tol2"] = round(out["surface_distance_sweep_ms"] / out["pr_sweep_tol2_ms"], 1)
    out["pr_tol2_faster_than_surface_distance"] = bool(out["pr_sweep_tol2_ms"] < out["surface_distance_sweep_ms"])
    return out


def leg_dataset(a):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet
    from csbsr_amd.data.synthetic import crack_masks
    from csbsr_amd.inference import evaluate_dataset
    from csbsr_amd.modeling.build_model import JointModel
    from csbsr_amd.utils.detfill import deterministic_fill
    model = JointModel(base_cfg.clone())
    deterministic_fill(model.state_dict())
    model.eval()
    hr, scale, B, n = 448, 4, 12, a.images
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, size=(hr, hr, 3), dtype=np.uint8) for _ in range(n)]
    lrs = [rng.integers(0, 256, size=(hr // scale, hr // scale, 3), dtype=np.uint8) for _ in range(n)]
    masks = [(m[0].numpy() * 255).astype(np.uint8) for m in crack_masks(n, hr, hr, torch.Generator().manual_seed(7))]
    r = np.arange(21) - 10
    gk = np.exp(-0.5 * ((r[None, :] / 1.5) ** 2 + (r[:, None] / 2.5) ** 2))
    kernels = [np.round(gk / gk.max() * 255).astype(np.uint8) for _ in range(n)]
    ts = ResidentTestSet(images, masks, lrs, kernels, [f"{i:03d}.jpg" for i in range(n)], device=DEV)

    def one_pass(tol):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evaluate_dataset(model, DeviceTestLoader(ts, hr, scale, B), pr_tolerance=tol)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), res
    _, with_pr = one_pass(2)
    _, without = one_pass(None)
    rates = {"with": [], "without": []}
    for _ in range(a.passes):
        rates["with"].append(round(one_pass(2)[0], 1))
        rates["without"].append(round(one_pass(None)[0], 1))
    return {"images": n, "hr": hr, "batch": B, "passes": a.passes, "images_per_s_with_pr_tolerance_2": rates["with"],
            "images_per_s_without": rates["without"], "best_with": max(rates["with"]), "best_without": max(rates["without"]),
            "iou_identical": bool(with_pr["iou"].tobytes() == without["iou"].tobytes()),
            "summary_pr": {k: round(with_pr["summary"][k], 6) for k in ("ODS", "ODS_threshold", "OIS", "AP", "P_at_ODS", "R_at_ODS")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sd-reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--legs", default="sweeps,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pr_sweep_bench.json"))
    a = ap.parse_args()
    assert a.reps >= 20 and a.sd_reps >= 1
    out = {"device": torch.cuda.get_device_name(0)}
    if "sweeps" in a.legs:
        out["sweeps"] = leg_sweeps(a)
    if "dataset" in a.legs:
        out["dataset"] = leg_dataset(a)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
