"""Time the crack topology (csrc/topology.hip): estimate_metrics.skeleton_topology and component_topology_table next to skeletonize and
label_components on the same masks in the same process, and predict_dataset with and without topology=True.

    python scripts/bench_topology.py                      # writes profiles/topology_bench.json and prints it as one JSON line

  kernels  the 8 maps of 1792^2 of scripts/bench_skeleton.py: the sparse crack masks at 0.5 and the model-like maps at 0.01 (about 31 % set).
           The topology is taken on the skeleton of each, and -- the dense case of the node kernel -- on the binarised plane itself.  Device
           events around ``reps`` calls after a warm-up, five such windows per call, the median reported with the spread (max / min - 1).
           A skeleton_topology call is the Python call: the topo and counts allocations, the counts' clear and the launch;
           csbsr_skeleton_topology alone is the entry on preallocated outputs.  component_topology_table includes component_table
           (csbsr_component_sums, the torch compaction), the labelling of the junction pixels and the gather; csbsr_component_topology alone
           is the entry.  A difference below the larger of two spreads is not a difference.
  dataset  predict_dataset without saving over synthetic LR images (stitched maps of 1792^2), config-2 model (deterministic fill): one
           warm-up pass each, then ``passes`` whole passes with measure_threshold and with measure_threshold + topology=True, alternating, the
           same with min_crack_px = 20.  ``parent_measure_images_per_s`` is the figure profiles/width_bench.json holds for the call without
           the option, measured before the option existed."""
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


def _ms(fn, a):
    med, spread, _ = windows(fn, a.reps, a.warmup)
    return {"ms": round(med, 4), "spread": round(spread, 4)}


def leg_kernels(a):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import _ptr
    from csbsr_amd.utils import estimate_metrics as EM
    prob, mask = crack_maps(a.maps, a.size)
    N, H, W = a.maps, a.size, a.size
    L.load()
    out = {"maps": N, "size": a.size, "reps": a.reps, "warmup": a.warmup, "windows": 5, "tile": [64, 128]}
    for tag, x, t in (("mask", mask, 0.5), ("pred_at_0.01", prob, 0.01)):
        x3 = x.reshape(N, H, W)
        r = {"set_fraction": round(float((x - t > 0).float().mean()), 5)}
        sk = EM.skeletonize(x3, t)
        labels = EM.label_components(x3, t)
        dense = (x3 - t > 0).to(torch.uint8)
        r["skeleton_px"] = int(sk.sum())
        for name, plane in (("skeleton", sk), ("region", dense)):
            topo, counts = EM.skeleton_topology(plane)
            again = EM.skeleton_topology(plane)
            comps = EM._count_roots(EM.label_components(plane.to(torch.float32), 0.5))
            juncs = EM._count_roots(EM._junction_labels(topo))
            s = [EM.summarize_topology(c, nc, nj) for c, nc, nj in zip(counts.cpu().numpy(), comps.cpu().tolist(), juncs.cpu().tolist())]
            e = _ms(lambda: EM.skeleton_topology(plane), a)
            t2, c2 = torch.empty_like(topo), torch.empty_like(counts)
            e["entry_ms"] = _ms(lambda: L.call("csbsr_skeleton_topology", _ptr(plane), N, H, W, _ptr(t2), _ptr(c2), L.stream(plane.device)), a)
            e.update(repeat_identical=bool(torch.equal(topo, again[0]) and torch.equal(counts, again[1])),
                     set_px=int(counts[:, 0].sum()), endpoints=sum(k["endpoints"] for k in s), junctions=sum(k["junctions"] for k in s),
                     junction_px=sum(k["junction_px"] for k in s), loops=sum(k["loops"] for k in s),
                     length_geodesic_px=round(sum(k["length_geodesic_px"] for k in s), 1),
                     gbytes_per_s_entry=round(2 * N * H * W / e["entry_ms"]["ms"] / 1e6, 1))
            r[f"skeleton_topology_{name}"] = e
        topo, _ = EM.skeleton_topology(sk)
        r["components"] = int(EM.component_topology_table(labels, topo).shape[0])
        r["component_topology_table"] = _ms(lambda: EM.component_topology_table(labels, topo), a)
        jl = EM._junction_labels(topo)
        tacc = torch.empty(N, EM.TOPO_ACC, H * W, dtype=torch.int32, device=labels.device)
        r["component_topology_kernels"] = _ms(lambda: L.call("csbsr_component_topology", _ptr(labels), _ptr(topo), _ptr(jl), N, H, W, _ptr(tacc),
                                                             L.stream(labels.device)), a)
        r["component_table"] = _ms(lambda: EM.component_table(labels, None), a)
        r["junction_labels"] = _ms(lambda: EM._junction_labels(topo), a)
        r["skeletonize"] = _ms(lambda: EM.skeletonize(x3, t), a)
        r["label_components"] = _ms(lambda: EM.label_components(x3, t), a)
        for name in ("skeleton", "region"):
            e = r[f"skeleton_topology_{name}"]
            e["skeletonize_over_topology"] = round(r["skeletonize"]["ms"] / e["ms"], 2)
            e["below_skeletonize_beyond_spread"] = bool(e["ms"] * (1 + max(e["spread"], r["skeletonize"]["spread"])) < r["skeletonize"]["ms"])
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
    t = float(first.float().median()) + 1e-3                 # bench_width.py's threshold: about half of this model's map is set
    t = min(max(t, 0.01), 0.99)
    modes = {"measure": dict(measure_threshold=t), "measure_topology": dict(measure_threshold=t, topology=True),
             "measure_min_crack_px_20": dict(measure_threshold=t, min_crack_px=20),
             "measure_min_crack_px_20_topology": dict(measure_threshold=t, min_crack_px=20, topology=True)}
    keys = ("crack_px", "skeleton_px", "n_cracks", "endpoints", "junctions", "junction_px", "isolated_px", "loops", "links", "length_geodesic_px",
            "orientation", "mean_width_px", "mean_width_geodesic_px")

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
    parent = None
    try:
        with open(os.path.join(ROOT, "profiles", "width_bench.json")) as fh:
            parent = json.load(fh)["dataset"]["median"]["measure"]
    except (OSError, KeyError, ValueError):
        pass
    med = {k: float(np.median(v)) for k, v in rates.items()}
    return {"images": a.images, "stitched": [4 * h, 4 * w], "passes": a.passes, "measure_threshold": round(t, 4),
            "set_fraction_image_0": round(float((first - t > 0).float().mean()), 5), "images_per_s": rates, "median": med,
            "spread": {k: round(max(v) / min(v) - 1, 4) for k, v in rates.items()},
            "cost_of_topology": {"measure": round(1 - med["measure_topology"] / med["measure"], 4),
                                 "measure_min_crack_px_20": round(1 - med["measure_min_crack_px_20_topology"] / med["measure_min_crack_px_20"], 4)},
            "parent_measure_images_per_s": parent, "image_0": {k: v[0] for k, v in last.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--legs", default="kernels,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topology_bench.json"))
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
