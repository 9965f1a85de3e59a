"""Time estimate_metrics.surface_distance_sweep (HD / MSD over the threshold sweep) per image: events after a warm-up, wall clock beside
them (the call synchronises once per image and once per threshold chunk and finishes on the host, so the two agree).

    python scripts/bench_surface_distance.py                       # the fixture's largest case, next to the reference's recorded seconds
    python scripts/bench_surface_distance.py --size 1792           # a sparse crack mask + perturbed prediction at config 2's HR size

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from csbsr_amd.utils.estimate_metrics import surface_distance_sweep  # noqa: E402
from csbsr_amd.inference import THRESHOLDS  # noqa: E402


def crack_case(size, seed=21):
    from csbsr_amd.data.synthetic import make_hr_mask
    _, mask = make_hr_mask(1, size, torch.Generator().manual_seed(seed))
    shifted = torch.roll(mask, (3, -2), (2, 3))
    prob = torch.nn.functional.avg_pool2d(shifted, 7, 1, 3)
    prob = (prob + 0.02 * torch.randn(prob.shape, generator=torch.Generator().manual_seed(seed + 1))).clamp(0, 1)
    return prob, mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=0, help="0: the fixture's largest random case")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workspace-mb", type=int, default=256)
    a = ap.parse_args()
    out = {}
    if a.size:
        prob, mask = crack_case(a.size)
        out["case"] = f"crack {a.size}x{a.size}"
    else:
        g = np.load(os.path.join(ROOT, "tests", "golden", "surface_distance.npz"))
        name = max(g["random_cases"], key=lambda n: g[f"prob_{n}"].size)
        prob = torch.from_numpy(g[f"prob_{name}"].astype(np.float32) / np.float32(255))[None, None]
        mask = torch.from_numpy(g[f"mask_{name}"].astype(np.float32))[None, None]
        out.update(case=str(name), reference_cpu_s_per_image=float(g[f"seconds_{name}"]))
    prob, mask = prob.cuda(), mask.cuda()
    kw = dict(workspace_bytes=a.workspace_mb << 20)
    for _ in range(2):
        r = surface_distance_sweep(prob, mask, THRESHOLDS, **kw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.reps):
        surface_distance_sweep(prob, mask, THRESHOLDS, **kw)
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / a.reps
    out.update(thresholds=len(THRESHOLDS), ms_per_image_events=round(e0.elapsed_time(e1) / a.reps, 3), ms_per_image_wall=round(wall * 1e3, 3),
               hd_median=float(np.median(r["hd"])), msd_median=float(np.median(r["msd"])), outliers=[r["hd_outliers"], r["msd_outliers"]])
    if "reference_cpu_s_per_image" in out:
        out["speedup_vs_reference"] = round(out["reference_cpu_s_per_image"] * 1e3 / out["ms_per_image_events"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
