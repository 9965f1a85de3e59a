"""Time the polyline simplification (csrc/simplify.hip): csbsr_polyline_simplify alone and estimate_metrics.simplify_polylines next to
order_branches and branch_polylines on the same tables in the same process, the host route they replace, predict_dataset with and without
simplify_px, and the length bias on rasterised straight lines.

    python scripts/bench_simplify.py                      # writes profiles/simplify_bench.json and prints it as one JSON line

  kernels  the tables of scripts/bench_polylines.py: the ordered points of the skeletons of 8 sparse crack masks of 1792^2 at 0.5 and of the
           model-like maps at 0.01 (about 31 % set: millions of chains of 1 to 3 points).  Device events around ``reps`` calls after a
           warm-up, five such windows per call, the median reported with the spread (max / min - 1).  simplify_entry_* is
           csbsr_polyline_simplify on preallocated arrays (its memset and two launches) at 0.5 / 1 / 2 px; simplify_polylines the Python call
           at 1 px: the allocations, the entry, the cumulative sum and the compaction.  A difference below the larger of two spreads is not
           a difference.
  host     the route the device path replaces: points and offsets copied to the host, then the NumPy recursion of tests/simplify_cases.py
           span by span, at 1 px -- a table of up to ``host_spans`` spans whole, of a larger one the spans of ONE image.  Wall clock, one
           run; the device entry is timed on all 8 images.
  dataset  predict_dataset without saving over synthetic LR images (stitched maps of 1792^2), config-2 model (deterministic fill): one
           warm-up pass each, then ``passes`` whole passes with measure_threshold + topology + branches + polylines and the same +
           simplify_px = 1.0, alternating.  ``polylines_again`` is a second series of the call without the option in the same loop: the gap
           between the two series of one configuration is the yardstick for a visible cost.
  bias     digital straight lines of 1000 columns at 0, 22.5 and 45 degrees (y = the row nearest to x tan(angle)) through
           simplify_polylines at 0.5 and at 1 px: the relative error of the simplified polyline's Euclidean length and of the chain code's
           arc_px against the distance between the line's ends.

Not measured: hardware counters, per-kernel traces, and several short spans packed into one wave."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_pr_sweep import DEV, crack_maps, windows  # noqa: E402

TOLERANCES = (0.5, 1.0, 2.0)


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
    out = {"maps": N, "size": a.size, "reps": a.reps, "warmup": a.warmup, "windows": 5, "route_limits": list(EM.SIMPLIFY_ROUTE_LIMITS)}
    for tag, x, t in (("mask", mask, 0.5), ("pred_at_0.01", prob, 0.01)):
        sk = EM.skeletonize(x.reshape(N, H, W), t)
        topo, _ = EM.skeleton_topology(sk)
        bl = EM.label_branches(topo)
        rank, diag = EM.order_branches(bl, topo)
        chain, offsets, points = EM.branch_polylines(bl, rank, diag)
        M, P = int(offsets.numel()) - 1, int(points.shape[0])
        px = torch.diff(offsets)
        lo, hi = EM.SIMPLIFY_ROUTE_LIMITS
        e = {"spans": M, "chains": int(chain.sum()), "points": P, "longest_chain_px": int(px.max()) if M else 0,
             "spans_by_route": {"wave": int((px <= lo).sum()), "lds": int(((px > lo) & (px <= hi)).sum()), "work": int((px > hi).sum())},
             "work_bytes": int(lib.csbsr_polyline_simplify_work_bytes(M, P))}
        st = L.stream(bl.device)
        work = torch.empty(e["work_bytes"], dtype=torch.uint8, device=bl.device)
        keep = torch.empty(P, dtype=torch.uint8, device=bl.device)
        vcount = torch.empty(M, dtype=torch.int32, device=bl.device)
        for tol in TOLERANCES:
            q = EM.simplify_tolerance(tol)
            call = lambda: L.call("csbsr_polyline_simplify", _ptr(offsets), _ptr(points), M, P, q, _ptr(work), _ptr(keep), _ptr(vcount), st)
            e[f"simplify_entry_{tol:g}px"] = _ms(call, a)
            first = keep.clone()
            call()
            e[f"vertices_{tol:g}px"] = int(keep.sum())
            e[f"repeat_identical_{tol:g}px"] = bool(torch.equal(first, keep)) and int(vcount.sum()) == e[f"vertices_{tol:g}px"]
        e["simplify_polylines_1px"] = _ms(lambda: EM.simplify_polylines(offsets, points, 1.0), a)
        e["order_branches"] = _ms(lambda: EM.order_branches(bl, topo), a)
        e["branch_polylines"] = _ms(lambda: EM.branch_polylines(bl, rank, diag), a)
        e["simplify_over_order_branches"] = round(e["simplify_polylines_1px"]["ms"] / e["order_branches"]["ms"], 3)
        n0 = M                                                   # a small table whole; of a large one the spans of image 0, whose pixels come first
        if M > a.host_spans:
            n0 = int(torch.searchsorted(offsets, int((rank[0] >= 0).sum()), right=True)) - 1
        e["host"] = leg_host(offsets[:n0 + 1], points[:int(offsets[n0])], EM.simplify_polylines(offsets, points, 1.0)[0])
        e["host"]["images"] = N if n0 == M else 1
        e["entry_all_images_below_host"] = e["simplify_entry_1px"]["ms"] < e["host"]["copy_ms"] + e["host"]["simplify_ms"]
        out[tag] = e
    return out


def leg_host(offsets, points, keep):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import simplify_cases as SV
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    off_h, pts_h = offsets.cpu().numpy(), points.cpu().numpy()
    t1 = time.perf_counter()
    k, v = SV.simplify_table(off_h, pts_h, 4, form=SV.simplify_stack)
    t2 = time.perf_counter()
    return {"spans": int(off_h.size - 1), "points": int(pts_h.shape[0]), "bytes_copied": int(off_h.nbytes + pts_h.nbytes), "copy_ms": round(1e3 * (t1 - t0), 2),
            "simplify_ms": round(1e3 * (t2 - t1), 2), "equals_the_device": bool(np.array_equal(k, keep[:pts_h.shape[0]].cpu().numpy()))}


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
    base = dict(measure_threshold=t, topology=True, branches=True, polylines=True)
    modes = {"polylines": base, "polylines_simplify": dict(simplify_px=1.0, **base), "polylines_again": base}
    keys = ("skeleton_px", "n_branches", "n_chains", "n_vertices", "length_simplified_px")

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
            "cost_of_simplify": round(1 - med["polylines_simplify"] / med["polylines"], 4),
            "same_configuration_twice": round(abs(1 - med["polylines_again"] / med["polylines"]), 4), "image_0": {k: v[0] for k, v in last.items()}}


def leg_bias(a):
    from csbsr_amd.utils import estimate_metrics as EM
    out = {"columns": a.line, "tolerances_px": [0.5, 1.0]}
    for deg in (0.0, 22.5, 45.0):
        slope = math.tan(math.radians(deg))
        yx = np.array([(int(math.floor(x * slope + 0.5)), x) for x in range(a.line)], np.int32)
        points = torch.from_numpy(np.concatenate([yx, np.zeros_like(yx)], 1)).to(DEV)
        offsets = torch.tensor([0, a.line], dtype=torch.int64, device=DEV)
        true = math.hypot(float(yx[-1, 0] - yx[0, 0]), float(yx[-1, 1] - yx[0, 1]))
        arc = EM.polyline_stats(yx)["arc_px"]
        e = {"true_px": round(true, 4), "arc_px": round(arc, 4), "pixel_count": a.line, "error_arc": round(arc / true - 1, 6),
             "error_pixel_count": round((a.line - 1) / true - 1, 6)}
        for tol in (0.5, 1.0):
            vindex = EM.simplify_polylines(offsets, points, tol)[2]
            simplified = EM.polyline_length(points[vindex.long()].cpu().numpy())
            e[f"at_{tol:g}px"] = {"vertices": int(vindex.numel()), "length_simplified_px": round(simplified, 4),
                                  "error_simplified": round(simplified / true - 1, 6)}
        out[f"{deg:g}_deg"] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--line", type=int, default=1001)
    ap.add_argument("--host_spans", type=int, default=100000)
    ap.add_argument("--legs", default="kernels,dataset,bias")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    if "kernels" in a.legs:
        out["kernels"] = leg_kernels(a)
    if "dataset" in a.legs:
        out["dataset"] = leg_dataset(a)
    if "bias" in a.legs:
        out["bias"] = leg_bias(a)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
