"""Time the crack branches (csrc/branches.hip): estimate_metrics.label_branches and branch_table next to label_components,
skeleton_topology and component_topology_table on the same masks in the same process, and predict_dataset with and without branches=True.

    python scripts/bench_branches.py                      # writes profiles/branches_bench.json and prints it as one JSON line

  kernels  the 8 maps of 1792^2 of scripts/bench_topology.py: the sparse crack masks at 0.5 and the model-like maps at 0.01 (about 31 % set).
           The branches are taken on the topo of each one's skeleton, and -- the dense case of the union-find -- on the topo of the binarised
           plane itself.  Device events around ``reps`` calls after a warm-up, five such windows per call, the median reported with the
           spread (max / min - 1).  label_branches is the Python call: the work and label allocations and the three launches;
           csbsr_branch_label alone is the entry on preallocated arrays.  branch_table includes csbsr_branch_sums, the torch compaction of the
           roots and the gathers; csbsr_branch_sums alone is the entry.  A difference below the larger of two spreads is not a difference.
  dataset  predict_dataset without saving over synthetic LR images (stitched maps of 1792^2), config-2 model (deterministic fill): one
           warm-up pass each, then ``passes`` whole passes with measure_threshold + topology and the same + branches=True, alternating, the
           same with min_crack_px = 20.  ``parent_topology_images_per_s`` is the figure profiles/prune_bench.json holds for the call without
           the option, measured before the option existed.

Not measured: hardware counters and per-kernel traces."""
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
        r["label_components"] = _ms(lambda: EM.label_components(x3, t), a)
        for name, plane in (("skeleton", sk), ("region", dense)):
            topo, counts = EM.skeleton_topology(plane)
            jl = EM._junction_labels(topo)
            bl, again = EM.label_branches(topo), EM.label_branches(topo)
            rows = EM.branch_table(bl, topo, jl, labels)
            s = EM.summarize_branches(rows)
            tiles = topo.view(N, H // 64, 64, W // 128, 128).ne(0).any(4).any(2) if H % 64 == 0 and W % 128 == 0 else None
            e = {"set_px": int(counts[:, 0].sum()), "junction_px": int(counts[:, 4].sum()), "branches": s["n_branches"], "kinds": s["branch_kinds"],
                 "longest_branch_px": round(s["longest_branch_px"], 1), "total_branch_px": round(s["total_branch_px"], 1),
                 "repeat_identical": bool(torch.equal(bl, again) and torch.equal(rows, EM.branch_table(bl, topo, jl, labels))),
                 "empty_tile_fraction": None if tiles is None else round(1.0 - float(tiles.float().mean()), 4)}
            e["label_branches"] = _ms(lambda: EM.label_branches(topo), a)
            work, b2 = torch.empty_like(bl), torch.empty_like(bl)
            e["branch_label_entry"] = _ms(lambda: L.call("csbsr_branch_label", _ptr(topo), N, H, W, _ptr(work), _ptr(b2), L.stream(topo.device)), a)
            e["branch_table"] = _ms(lambda: EM.branch_table(bl, topo, jl, labels), a)
            bacc = torch.empty(N, EM.BRANCH_ACC, H * W, dtype=torch.int32, device=bl.device)
            e["branch_sums_entry"] = _ms(lambda: L.call("csbsr_branch_sums", _ptr(bl), _ptr(topo), _ptr(jl), None, N, H, W, _ptr(bacc),
                                                        L.stream(bl.device)), a)
            e["skeleton_topology"] = _ms(lambda: EM.skeleton_topology(plane), a)
            e["junction_labels"] = _ms(lambda: EM._junction_labels(topo), a)
            lab8 = labels if name == "skeleton" else EM.label_components(plane.to(torch.float32), 0.5)
            e["component_topology_table"] = _ms(lambda: EM.component_topology_table(lab8, topo), a)
            # the labelling reads a byte and writes work, then reads work and writes the labels: 13 bytes a pixel
            e["gbytes_per_s_label_entry"] = round(13 * N * H * W / e["branch_label_entry"]["ms"] / 1e6, 1)
            e["label_branches_over_label_components"] = round(e["label_branches"]["ms"] / r["label_components"]["ms"], 3)
            e["branch_table_over_component_topology_table"] = round(e["branch_table"]["ms"] / e["component_topology_table"]["ms"], 3)
            e["label_branches_over_skeleton_topology"] = round(e["label_branches"]["ms"] / e["skeleton_topology"]["ms"], 3)
            r[name] = e
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
    modes = {"topology": dict(measure_threshold=t, topology=True), "topology_branches": dict(measure_threshold=t, topology=True, branches=True),
             "min_crack_px_20_topology": dict(measure_threshold=t, min_crack_px=20, topology=True),
             "min_crack_px_20_topology_branches": dict(measure_threshold=t, min_crack_px=20, topology=True, branches=True)}
    keys = ("crack_px", "skeleton_px", "n_cracks", "endpoints", "junctions", "loops", "length_geodesic_px", "n_branches", "branch_kinds",
            "longest_branch_px")

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
        with open(os.path.join(ROOT, "profiles", "prune_bench.json")) as fh:
            parent = json.load(fh)["dataset"]["median"]
    except (OSError, KeyError, ValueError):
        pass
    med = {k: float(np.median(v)) for k, v in rates.items()}
    spread = {k: round(max(v) / min(v) - 1, 4) for k, v in rates.items()}
    out = {"images": a.images, "stitched": [4 * h, 4 * w], "passes": a.passes, "measure_threshold": round(t, 4),
           "set_fraction_image_0": round(float((first - t > 0).float().mean()), 5), "images_per_s": rates, "median": med, "spread": spread,
           "cost_of_branches": {"topology": round(1 - med["topology_branches"] / med["topology"], 4),
                                "min_crack_px_20_topology": round(1 - med["min_crack_px_20_topology_branches"] / med["min_crack_px_20_topology"], 4)},
           "image_0": {k: v[0] for k, v in last.items()}}
    if parent is not None:
        out["parent_images_per_s"] = {k: parent.get(k) for k in ("topology", "min_crack_px_20_topology")}
        out["without_the_option_vs_parent"] = {k: {"ratio": round(med[k] / parent[k], 4), "inside_the_spread": bool(abs(med[k] / parent[k] - 1) <= spread[k])}
                                               for k in ("topology", "min_crack_px_20_topology") if parent.get(k)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--legs", default="kernels,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branches_bench.json"))
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
