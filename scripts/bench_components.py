"""Time the connected components (csrc/components.hip): estimate_metrics.label_components, component_table and keep_components next to
skeletonize and pr_sweep on the same tensors in the same process, the kernels of csbsr_component_sums by themselves, and predict_dataset
with and without min_crack_px.

    python scripts/bench_components.py                    # writes profiles/components_bench.json and prints it as one JSON line

  kernels  the 8 maps of 1792^2 of scripts/bench_pr_sweep.py, binarised three ways: the sparse crack masks at 0.5, the model-like maps at 0.5
           and at 0.01 (about 31 % set: the blurred cracks and a good part of the noise floor -- many small components and long runs).
           Device events around ``reps`` calls after a warm-up, five such windows per call, the median reported with the spread (max / min
           - 1).  A label_components call is the Python call: the scratch and label allocations and the three launches.  component_table
           includes the torch compaction (nonzero, gather); ``sums_kernels`` is csbsr_component_sums alone (root reset + accumulation: one
           lane per pixel, one atomic add per horizontal run inside a wave, the box atomics only where a relaxed load says they would change).
  dataset  predict_dataset without saving over synthetic LR images (stitched maps of 1792^2), config-2 model (deterministic fill): one
           warm-up pass each, then whole passes without measuring, with measure_threshold, and with measure_threshold + min_crack_px,
           alternating."""
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
    lib = L.load()
    import ctypes
    th, tw = ctypes.c_int32(0), ctypes.c_int32(0)
    lib.csbsr_ccl_tile(ctypes.byref(th), ctypes.byref(tw))
    out = {"maps": N, "size": a.size, "reps": a.reps, "warmup": a.warmup, "tile": [th.value, tw.value],
           "merge": "one launch over all seam pixels, agent-scope atomic min (the hierarchical form: unmeasured)"}
    for tag, x, t in (("mask", mask, 0.5), ("pred", prob, 0.5), ("pred_at_0.01", prob, 0.01)):
        r = {"set_fraction": round(float((x - t > 0).float().mean()), 5)}
        for conn in (8, 4):
            med, spread, _ = windows(lambda: EM.label_components(x, t, conn), a.reps, a.warmup)
            r[f"label_components_{conn}"] = {"ms": round(med, 4), "spread": round(spread, 4)}
        labels = EM.label_components(x, t)
        r["repeat_identical"] = bool(torch.equal(labels, EM.label_components(x, t)))
        sk = EM.skeletonize(x, t)
        table = EM.component_table(labels, sk)
        r["components"] = int(table.shape[0])
        r["largest_area_px"] = int(table[:, 2].max()) if table.shape[0] else 0
        r["components_of_20_px_or_more"] = int((table[:, 2] >= 20).sum())
        med, spread, _ = windows(lambda: EM.component_table(labels, sk), a.reps, a.warmup)
        r["component_table"] = {"ms": round(med, 4), "spread": round(spread, 4)}
        acc = torch.empty(N, EM.CC_ACC, H * W, dtype=torch.int32, device=labels.device)
        med, spread, _ = windows(lambda: L.call("csbsr_component_sums", _ptr(labels), _ptr(sk), N, H, W, _ptr(acc), L.stream(labels.device)),
                                 a.reps, a.warmup)
        r["sums_kernels"] = {"ms": round(med, 4), "spread": round(spread, 4), "ns_per_component": round(1e6 * med / max(1, table.shape[0]), 3)}
        med, spread, _ = windows(lambda: EM.keep_components(labels, 20), a.reps, a.warmup)
        r["keep_components_20"] = {"ms": round(med, 4), "spread": round(spread, 4)}
        med, spread, _ = windows(lambda: EM.skeletonize(x, t), a.reps, a.warmup)
        r["skeletonize"] = {"ms": round(med, 4), "spread": round(spread, 4)}
        out[tag] = r
    med, spread, _ = windows(lambda: EM.pr_sweep(prob, mask, THRESHOLDS, 2), a.reps, a.warmup)
    out["pr_sweep_tol2"] = {"ms": round(med, 4), "spread": round(spread, 4)}
    med, spread, _ = windows(lambda: EM.iou_sweep(prob, mask, THRESHOLDS), a.reps, a.warmup)
    out["iou_sweep"] = {"ms": round(med, 4), "spread": round(spread, 4)}
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
    t = float(first.float().median()) + 1e-3                 # a threshold that sets about half of this model's map: a hard plane for the labelling
    t = min(max(t, 0.01), 0.99)
    modes = {"plain": {}, "measure": dict(measure_threshold=t), "measure_min_crack_px_20": dict(measure_threshold=t, min_crack_px=20)}

    def one_pass(kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = [{k: v for k, v in d.items() if k in ("crack_px", "skeleton_px", "removed_px", "n_cracks")} for d in predict_dataset(model, ld, **kw)]
        torch.cuda.synchronize()
        return a.images / (time.perf_counter() - t0), res
    last = {k: one_pass(kw)[1] for k, kw in modes.items()}
    rates = {k: [] for k in modes}
    for _ in range(a.passes):
        for k, kw in modes.items():
            rates[k].append(round(one_pass(kw)[0], 2))
    return {"images": a.images, "stitched": [4 * h, 4 * w], "passes": a.passes, "measure_threshold": round(t, 4),
            "set_fraction_image_0": round(float((first - t > 0).float().mean()), 5), "images_per_s": rates,
            "median": {k: float(np.median(v)) for k, v in rates.items()}, "image_0": {k: v[0] for k, v in last.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--legs", default="kernels,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
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
