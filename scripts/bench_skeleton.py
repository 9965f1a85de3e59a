"""Time the centerline metrics (csrc/skeleton.hip): estimate_metrics.skeletonize and centerline_counts next to pr_sweep and iou_sweep on the
same tensors in the same process, one launch of csbsr_skeleton_passes by itself, and evaluate_dataset with and without cldice_threshold.

    python scripts/bench_skeleton.py                      # writes profiles/skeleton_bench.json and prints it as one JSON line

  kernels  the 8 maps of 1792^2 of scripts/bench_pr_sweep.py: sparse synthetic crack masks and model-like maps.  Device events around
           ``reps`` calls after a warm-up, five such windows per call, the median reported with the spread (max / min - 1).  A skeletonize call
           is the Python call: two work plane sets, init, the launch groups with one 4-byte read-back each, finish.  ``passes_launch`` is
           one csbsr_skeleton_passes launch of the full number of passes on the freshly binarised planes, without the read-back.
           Only the bit-packed LDS form was built; a byte-per-pixel form is unmeasured.
  dataset  evaluate_dataset without saving over 48 synthetic 448^2 images, config-2 model (deterministic fill), batch 12: one warm-up pass
           each, then five whole passes with cldice_threshold = 0.5 and five without, alternating."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_pr_sweep import DEV, crack_maps, windows  # noqa: E402


def leg_kernels(a):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import _ptr
    from csbsr_amd.inference import THRESHOLDS
    from csbsr_amd.utils import estimate_metrics as EM
    prob, mask = crack_maps(a.maps, a.size)
    N, H, W = a.maps, a.size, a.size
    out = {"maps": N, "size": a.size, "reps": a.reps, "warmup": a.warmup, "representation": "one bit per pixel in LDS (byte per pixel: unmeasured)",
           "passes_per_launch": int(L.load().csbsr_skeleton_max_passes()), "gt_fraction": round(float((mask > 0.5).float().mean()), 5),
           "pred_fraction_at_0.5": round(float((prob - 0.5 > 0).float().mean()), 5)}
    for tag, x in (("mask", mask), ("pred", prob)):
        sk, groups, passes, deleted = EM._thin(x, 0.5, 0)
        again = EM._thin(x, 0.5, 0)[0]
        med, spread, _ = windows(lambda: EM.skeletonize(x, 0.5), a.reps, a.warmup)
        out[f"skeletonize_{tag}"] = {"ms": round(med, 4), "spread": round(spread, 4), "launch_groups": groups, "passes_launched": passes,
                                     "pixels_deleted": deleted, "skeleton_px": int(sk.sum()), "repeat_identical": bool(torch.equal(sk, again)),
                                     "us_per_pass_per_plane": round(1e3 * med / (passes * N), 3)}
    ww = (W + 31) // 32
    wa, wb = (torch.empty(N, H, ww, dtype=torch.int32, device=DEV) for _ in range(2))
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    K = out["passes_per_launch"]
    for tag, x, t in (("mask", mask, 0.5), ("pred_at_0.01", prob, 0.01)):
        L.call("csbsr_skeleton_init", _ptr(x), t, N, H, W, _ptr(wa), L.stream(x.device))
        med, spread, _ = windows(lambda: L.call("csbsr_skeleton_passes", _ptr(wa), _ptr(wb), N, H, W, K, _ptr(cnt), L.stream(x.device)), a.reps, a.warmup)
        out[f"passes_launch_{tag}"] = {"ms": round(med, 4), "spread": round(spread, 4), "set_fraction": round(float((x - t > 0).float().mean()), 5),
                                       "us_per_pass_per_plane": round(1e3 * med / (K * N), 3)}
    med, spread, _ = windows(lambda: EM.centerline_counts(prob, mask, 0.5), a.reps, a.warmup)
    out["centerline_counts"] = {"ms": round(med, 4), "spread": round(spread, 4), "counts_image_0": EM.centerline_counts(prob, mask, 0.5)[0].tolist()}
    sp, sl = EM.skeletonize(prob, 0.5), EM.skeletonize(mask, 0.5)
    c = torch.empty(N, 4, dtype=torch.int32, device=DEV)
    med, spread, _ = windows(lambda: L.call("csbsr_centerline_counts", _ptr(sp), _ptr(prob), 0.5, _ptr(sl), _ptr(mask), N, H, W, _ptr(c),
                                            L.stream(prob.device)), a.reps, a.warmup)
    out["centerline_counts_kernel_only"] = {"ms": round(med, 4), "spread": round(spread, 4), "GBps": round(10 * prob.numel() / (med * 1e-3) / 1e9, 1)}
    med, spread, _ = windows(lambda: EM.pr_sweep(prob, mask, THRESHOLDS, 2), a.reps, a.warmup)
    out["pr_sweep_tol2"] = {"ms": round(med, 4), "spread": round(spread, 4)}
    med, spread, _ = windows(lambda: EM.iou_sweep(prob, mask, THRESHOLDS), a.reps, a.warmup)
    out["iou_sweep"] = {"ms": round(med, 4), "spread": round(spread, 4)}
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

    def one_pass(t):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = evaluate_dataset(model, DeviceTestLoader(ts, hr, scale, B), cldice_threshold=t)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0), res
    _, with_cl = one_pass(0.5)
    _, without = one_pass(None)
    rates = {"with": [], "without": []}
    for _ in range(a.passes):
        rates["with"].append(round(one_pass(0.5)[0], 1))
        rates["without"].append(round(one_pass(None)[0], 1))
    return {"images": n, "hr": hr, "batch": B, "passes": a.passes, "images_per_s_with_cldice_threshold_0.5": rates["with"],
            "images_per_s_without": rates["without"], "median_with": float(np.median(rates["with"])),
            "median_without": float(np.median(rates["without"])), "iou_identical": bool(with_cl["iou"].tobytes() == without["iou"].tobytes()),
            "summary_cldice": {k: round(with_cl["summary"][k], 6) for k in ("clDice", "Tprec", "Tsens", "clDice_pooled")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--legs", default="kernels,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skeleton_bench.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if "kernels" in a.legs:
        out["kernels"] = leg_kernels(a)
    if "dataset" in a.legs:
        out["dataset"] = leg_dataset(a)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
