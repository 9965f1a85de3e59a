"""Time the local crack width (csrc/width.hip): estimate_metrics.skeleton_width at r = 16, 64 and 128 and component_width_table next to
skeletonize, label_components and the dense exact distance transform csbsr_sdf on the same masks in the same process, and predict_dataset
with and without width_radius.

    python scripts/bench_width.py                         # writes profiles/width_bench.json and prints it as one JSON line

  kernels  the 8 maps of 1792^2 of scripts/bench_components.py: the sparse crack masks at 0.5 and the model-like maps at 0.01 (about 31 % set).
           Device events around ``reps`` calls after a warm-up, five such windows per call, the median reported with the spread (max / min
           - 1).  A skeleton_width call is the Python call: the d2 and histogram allocations, the histogram's clear and the launch.
           component_width_table includes component_table (csbsr_component_sums, the torch compaction) and the gather.  csbsr_sdf is the
           yardstick: the dense route to the same distances that existing parts offer (two exact transforms and a combine pass, fp32).
           A difference below the larger of two spreads is not a difference.
  dataset  predict_dataset without saving over synthetic LR images (stitched maps of 1792^2), config-2 model (deterministic fill): one
           warm-up pass each, then five whole passes with measure_threshold and with measure_threshold + width_radius = 64, alternating, the
           same with min_crack_px = 20."""
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

RADII = (16, 64, 128)


def _ms(fn, a):
    med, spread, _ = windows(fn, a.reps, a.warmup)
    return {"ms": round(med, 4), "spread": round(spread, 4)}


def leg_kernels(a):
    import ctypes
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import _ptr
    from csbsr_amd.utils import estimate_metrics as EM
    prob, mask = crack_maps(a.maps, a.size)
    N, H, W = a.maps, a.size, a.size
    lib = L.load()
    th, tw = ctypes.c_int32(0), ctypes.c_int32(0)
    lib.csbsr_width_tile(ctypes.byref(th), ctypes.byref(tw))
    out = {"maps": N, "size": a.size, "reps": a.reps, "warmup": a.warmup, "windows": 5, "tile": [th.value, tw.value]}
    for tag, x, t in (("mask", mask, 0.5), ("pred_at_0.01", prob, 0.01)):
        x3 = x.reshape(N, H, W)
        r = {"set_fraction": round(float((x - t > 0).float().mean()), 5)}
        sk = EM.skeletonize(x3, t)
        labels = EM.label_components(x3, t)
        r["skeleton_px"] = int(sk.sum())
        r["skeleton_fraction"] = round(r["skeleton_px"] / sk.numel(), 6)
        tiles = sk.view(N, H // th.value, th.value, W // tw.value, tw.value).amax(dim=(2, 4)) if H % th.value == 0 and W % tw.value == 0 else None
        r["tiles_with_skeleton_fraction"] = None if tiles is None else round(float(tiles.float().mean()), 4)
        for rad in RADII:
            d2, hist = EM.skeleton_width(x3, sk, t, rad)
            again = EM.skeleton_width(x3, sk, t, rad)
            s = EM.summarize_width_hist(hist.sum(0), rad)
            e = _ms(lambda: EM.skeleton_width(x3, sk, t, rad), a)
            e.update(repeat_identical=bool(torch.equal(d2, again[0]) and torch.equal(hist, again[1])), saturated_px=s["saturated_px"],
                     median_width_px=round(s["median_width_px"], 3), p95_width_px=round(s["p95_width_px"], 3), max_width_px=round(s["max_width_px"], 3))
            r[f"skeleton_width_r{rad}"] = e
        d2, _ = EM.skeleton_width(x3, sk, t, 64)
        r["components"] = int(EM.component_width_table(labels, d2).shape[0])
        r["component_width_table"] = _ms(lambda: EM.component_width_table(labels, d2), a)
        wacc = torch.empty(N, 2, H * W, dtype=torch.int32, device=labels.device)
        r["component_width_kernels"] = _ms(lambda: L.call("csbsr_component_width", _ptr(labels), _ptr(d2), N, H, W, _ptr(wacc), L.stream(labels.device)), a)
        r["skeletonize"] = _ms(lambda: EM.skeletonize(x3, t), a)
        r["label_components"] = _ms(lambda: EM.label_components(x3, t), a)
        # the dense yardstick, on the same binary plane (csbsr_sdf reads a mask: > 0.5)
        m = (x3 - t > 0).to(torch.float32).view(N, 1, H, W).contiguous()
        sdf, scratch = torch.empty_like(m), torch.empty(3 * N * H * W + 2 * N, dtype=torch.float32, device=m.device)
        r["csbsr_sdf"] = _ms(lambda: L.call("csbsr_sdf", _ptr(m), _ptr(sdf), _ptr(scratch), N, H, W, L.stream(m.device)), a)
        for rad in RADII:
            e = r[f"skeleton_width_r{rad}"]
            e["sdf_over_width"] = round(r["csbsr_sdf"]["ms"] / e["ms"], 2)
            e["faster_than_sdf_beyond_spread"] = bool(e["ms"] * (1 + max(e["spread"], r["csbsr_sdf"]["spread"])) < r["csbsr_sdf"]["ms"])
        out[tag] = r
    return out


def leg_dataset(a):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd.inference import predict_dataset
    from csbsr_amd.modeling.build_model import JointModel
    from csbsr_amd.utils.detfill import deterministic_fill
    model = JointModel(base_cfg.clone())
    deterministic_fill(model.state_dict())
    model.eval()
    h = w = a.size // 4
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(a.images)]
    ld = DevicePredictLoader(ResidentImageSet(images, [f"{i:03d}.png" for i in range(a.images)], device=DEV), 64, 4, halo=0, batch_patches=16)
    first = next(predict_dataset(model, ld))["map_f32"]
    t = float(first.float().median()) + 1e-3                 # bench_components.py's threshold: about half of this model's map is set
    t = min(max(t, 0.01), 0.99)
    modes = {"measure": dict(measure_threshold=t), "measure_width_64": dict(measure_threshold=t, width_radius=64),
             "measure_min_crack_px_20": dict(measure_threshold=t, min_crack_px=20),
             "measure_min_crack_px_20_width_64": dict(measure_threshold=t, min_crack_px=20, width_radius=64)}
    keys = ("crack_px", "skeleton_px", "n_cracks", "max_width_px", "median_width_px", "p95_width_px", "saturated_px", "widest")

    def one_pass(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = [{k: v for k, v in d.items() if k in keys} for d in predict_dataset(model, ld, **kw)]
        torch.cuda.synchronize()
        return a.images / (time.perf_counter() - t0), res
    last = {k: one_pass(kw)[1] for k, kw in modes.items()}
    rates = {k: [] for k in modes}
    for _ in range(a.passes):
        for k, kw in modes.items():
            rates[k].append(round(one_pass(kw)[0], 2))
    return {"images": a.images, "stitched": [4 * h, 4 * w], "passes": a.passes, "measure_threshold": round(t, 4),
            "set_fraction_image_0": round(float((first - t > 0).float().mean()), 5), "images_per_s": rates,
            "median": {k: float(np.median(v)) for k, v in rates.items()},
            "spread": {k: round(max(v) / min(v) - 1, 4) for k, v in rates.items()}, "image_0": {k: v[0] for k, v in last.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--legs", default="kernels,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "width_bench.json"))
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
