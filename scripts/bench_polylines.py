"""Time the crack polylines (csrc/polylines.hip): estimate_metrics.order_branches and branch_polylines next to label_branches, branch_table
and skeleton_topology on the same skeletons in the same process, the host walk they replace, and predict_dataset with and without
polylines=True.

    python scripts/bench_polylines.py                     # writes profiles/polylines_bench.json and prints it as one JSON line

  kernels  the 8 maps of 1792^2 of scripts/bench_branches.py: the sparse crack masks at 0.5 and the model-like maps at 0.01 (about 31 % set),
           each one's skeleton.  Device events around ``reps`` calls after a warm-up, five such windows per call, the median reported with
           the spread (max / min - 1).  order_branches is the Python call: the count, its 8-byte read, the allocations and the R + 4
           launches; branch_order_entry alone is csbsr_branch_order on preallocated arrays with the count known.  per_round is the entry
           with the list sized for 4 P -- two more jump launches over the same list -- minus the entry itself, halved.  A difference below
           the larger of two spreads is not a difference.
  host     the route the device path replaces, for ONE image of 1792^2: branch_map and topology_map copied to the host (5 bytes a pixel),
           then the NumPy walk of tests/polyline_cases.py.  Wall clock, one run.
  dataset  predict_dataset without saving over synthetic LR images (stitched maps of 1792^2), config-2 model (deterministic fill): one
           warm-up pass each, then ``passes`` whole passes with measure_threshold + topology + branches and the same + polylines=True,
           alternating.  ``branches_again`` is a second series of the call without the option in the same loop: the gap between the two
           series of one configuration is the yardstick for a visible cost.

Not measured: hardware counters, per-kernel traces, and a tile-local pre-ranking in LDS."""
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
    lib = L.load()
    out = {"maps": N, "size": a.size, "reps": a.reps, "warmup": a.warmup, "windows": 5, "tile": [64, 128]}
    for tag, x, t in (("mask", mask, 0.5), ("pred_at_0.01", prob, 0.01)):
        x3 = x.reshape(N, H, W)
        sk = EM.skeletonize(x3, t)
        topo, counts = EM.skeleton_topology(sk)
        jl = EM._junction_labels(topo)
        bl = EM.label_branches(topo)
        rank, diag, R = EM.order_branches(bl, topo, return_rounds=True)
        again = EM.order_branches(bl, topo)
        chain, offsets, points = EM.branch_polylines(bl, rank, diag)
        px = torch.diff(offsets)
        P = int((bl != 0).sum())
        e = {"set_fraction": round(float((x - t > 0).float().mean()), 5), "skeleton_px": int(counts[:, 0].sum()), "branch_px": P,
             "branches": int(chain.numel()), "chains": int(chain.sum()), "ordered_px": int(points.shape[0]),
             "unordered_px": P - int(points.shape[0]), "longest_chain_px": int(px.max()) if px.numel() else 0, "rounds": R, "launches": R + 4,
             "work_bytes": int(lib.csbsr_branch_order_work_bytes(P)),
             "repeat_identical": bool(torch.equal(rank, again[0]) and torch.equal(diag, again[1]))}
        e["order_branches"] = _ms(lambda: EM.order_branches(bl, topo), a)
        st = L.stream(bl.device)
        r2, d2 = torch.empty_like(rank), torch.empty_like(diag)
        for key, cap in (("branch_order_entry", P), ("branch_order_entry_4P", 4 * P)):
            work = torch.empty(int(lib.csbsr_branch_order_work_bytes(cap)), dtype=torch.uint8, device=bl.device)
            e[key] = _ms(lambda: L.call("csbsr_branch_order", _ptr(topo), _ptr(bl), N, H, W, cap, _ptr(work), _ptr(r2), _ptr(d2), st), a)
            assert torch.equal(r2, rank) and torch.equal(d2, diag)
        e["per_round_ms"] = round((e["branch_order_entry_4P"]["ms"] - e["branch_order_entry"]["ms"]) / 2, 4)
        count = torch.empty(1, dtype=torch.int64, device=bl.device)
        e["branch_count_entry"] = _ms(lambda: L.call("csbsr_branch_count", _ptr(topo), N, H, W, _ptr(count), st), a)
        e["branch_polylines"] = _ms(lambda: EM.branch_polylines(bl, rank, diag), a)
        first = torch.zeros(N * H * W, dtype=torch.int32, device=bl.device)
        e["branch_scatter_entry"] = _ms(lambda: L.call("csbsr_branch_scatter", _ptr(bl), _ptr(rank), _ptr(diag), None, _ptr(first), N, H, W,
                                                       int(points.shape[0]), _ptr(points), st), a)
        e["label_branches"] = _ms(lambda: EM.label_branches(topo), a)
        e["branch_table"] = _ms(lambda: EM.branch_table(bl, topo, jl), a)
        e["skeleton_topology"] = _ms(lambda: EM.skeleton_topology(sk), a)
        e["order_branches_over_label_branches"] = round(e["order_branches"]["ms"] / e["label_branches"]["ms"], 3)
        e["order_entry_over_label_branches"] = round(e["branch_order_entry"]["ms"] / e["label_branches"]["ms"], 3)
        out[tag] = e
        if tag == "mask":
            out["host_walk_one_image"] = leg_host(bl[0], topo[0], rank[0], diag[0])
    return out


def leg_host(bl, topo, rank, diag):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import polyline_cases as PC
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bl_h, topo_h = bl.cpu().numpy(), topo.cpu().numpy()
    t1 = time.perf_counter()
    r, d = PC.walk(topo_h, bl_h)
    t2 = time.perf_counter()
    return {"bytes_copied": int(bl_h.nbytes + topo_h.nbytes), "branch_px": int((bl_h != 0).sum()), "copy_ms": round(1e3 * (t1 - t0), 2),
            "walk_ms": round(1e3 * (t2 - t1), 2), "equals_the_device": bool(np.array_equal(r, rank.cpu().numpy()) and np.array_equal(d, diag.cpu().numpy()))}


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
    base = dict(measure_threshold=t, topology=True, branches=True)
    modes = {"branches": base, "branches_polylines": dict(polylines=True, **base), "branches_again": base}
    keys = ("skeleton_px", "n_branches", "n_chains", "unordered_branch_px")

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
            rates[k].append(round(one_pass(kw)[0], 3))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    spread = {k: round(max(v) / min(v) - 1, 4) for k, v in rates.items()}
    return {"images": a.images, "stitched": [4 * h, 4 * w], "passes": a.passes, "measure_threshold": round(t, 4),
            "set_fraction_image_0": round(float((first - t > 0).float().mean()), 5), "images_per_s": rates, "median": med, "spread": spread,
            "cost_of_polylines": round(1 - med["branches_polylines"] / med["branches"], 4),
            "same_configuration_twice": round(abs(1 - med["branches_again"] / med["branches"]), 4), "image_0": {k: v[0] for k, v in last.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--legs", default="kernels,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polylines_bench.json"))
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
