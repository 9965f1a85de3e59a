"""Time the crack gap bridging (csrc/gaps.hip): estimate_metrics.endpoint_gaps at G = 4, 16 and 64, gap_groups and draw_bridges next to
skeleton_width(r = 64) and skeleton_topology on the same masks in the same process, the host route it replaces for one image, and
predict_dataset with and without bridge_gap_px.

    python scripts/bench_gaps.py                          # writes profiles/gaps_bench.json and prints it as one JSON line

  kernels  the 8 maps of 1792^2 of scripts/bench_width.py: the sparse crack masks at 0.5 and the model-like maps at 0.01 (about 31 % set).
           Device events around ``reps`` calls after a warm-up, five such windows per call, the median reported with the spread (max / min
           - 1).  A call is the Python call: the output allocations and the launches.  A call that takes longer than 50 ms is timed with
           2 calls per window, one that takes longer than a second once.  A difference below the larger of two spreads is not a difference.
  host     for ONE image of the sparse masks: the copy of its topo bytes and labels to the host (16 MB at 1792^2) and the vectorised NumPy
           search of the restatement (sources against targets, the 64-bit key), whose result is compared with the device's.
  dataset  predict_dataset without saving over synthetic LR images (stitched maps of 1792^2), config-2 model (deterministic fill): one
           warm-up pass each, then whole passes with measure_threshold + topology, the same with bridge_gap_px = 16, and the first
           configuration again, alternating; one more pass with bridge_gap_px = 64."""
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

GAPS = (4, 16, 64)


def _ms(fn, a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    once = time.perf_counter() - t0
    if once > 1.0:                                           # seconds per call: the one call is the measurement
        return {"ms": round(once * 1e3, 1), "spread": None, "calls_per_window": 1}
    slow = once > 0.05
    med, spread, _ = windows(fn, 2 if slow else a.reps, 1 if slow else a.warmup)
    return {"ms": round(med, 4), "spread": round(spread, 4), "calls_per_window": 2 if slow else a.reps}


def host_search(topo, labels, G):
    """the NumPy restatement for one plane: (gap_q, gap_d2), every source against every target of the plane"""
    H, W = topo.shape
    cls = topo & 7
    src, tgt = ((cls == 1) | (cls == 2)) & (labels != 0), (cls != 0) & (labels != 0)
    gq, gd = np.full((H, W), -1, np.int32), np.zeros((H, W), np.int32)
    sy, sx = np.nonzero(src)
    ty, tx = np.nonzero(tgt)
    if len(sy) and len(ty):
        tl, tq = labels[ty, tx], (ty * W + tx).astype(np.int64)
        none = np.int64((G * G + 1) << 32)
        for a in range(0, len(sy), 256):
            y, x = sy[a:a + 256, None].astype(np.int64), sx[a:a + 256, None].astype(np.int64)
            d2 = (ty[None] - y) ** 2 + (tx[None] - x) ** 2
            key = np.where((d2 <= G * G) & (tl[None] != labels[sy[a:a + 256], sx[a:a + 256]][:, None]), (d2 << 32) | tq[None], none).min(1)
            has = key < none
            gq[sy[a:a + 256][has], sx[a:a + 256][has]] = (key[has] & 0xFFFFFFFF).astype(np.int32)
            gd[sy[a:a + 256][has], sx[a:a + 256][has]] = (key[has] >> 32).astype(np.int32)
    return gq, gd


def leg_host(topo, labels, gq_dev, G):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    topo_h, labels_h = topo.cpu().numpy(), labels.cpu().numpy()
    t1 = time.perf_counter()
    gq, gd = host_search(topo_h, labels_h, G)
    t2 = time.perf_counter()
    return {"G": G, "bytes_copied": int(topo_h.nbytes + labels_h.nbytes), "sources": int((((topo_h & 7) == 1) | ((topo_h & 7) == 2)).sum()),
            "gaps": int((gq >= 0).sum()), "copy_ms": round((t1 - t0) * 1e3, 3), "search_ms": round((t2 - t1) * 1e3, 3),
            "equals_the_device": bool(np.array_equal(gq, gq_dev.cpu().numpy()))}


def leg_kernels(a):
    from csbsr_amd.utils import estimate_metrics as EM
    prob, mask = crack_maps(a.maps, a.size)
    N, H, W = a.maps, a.size, a.size
    out = {"maps": N, "size": a.size, "reps": a.reps, "warmup": a.warmup, "windows": 5, "tile": [64, 128]}
    for tag, x, t in (("mask", mask, 0.5), ("pred_at_0.01", prob, 0.01)):
        x3 = x.reshape(N, H, W)
        sk = EM.skeletonize(x3, t)
        labels = EM.label_components(x3, t)
        topo, counts = EM.skeleton_topology(sk)
        cls = topo & 7
        src = (cls == 1) | (cls == 2)
        r = {"set_fraction": round(float((x - t > 0).float().mean()), 5), "skeleton_px": int(sk.sum()), "sources": int(src.sum()),
             "components": int(EM._count_roots(labels).sum()),
             "tiles_with_a_source_fraction": round(float(src.view(N, H // 64, 64, W // 128, 128).amax(dim=(2, 4)).float().mean()), 4)}
        for G in GAPS:
            for to in ("any", "end"):
                gq, gd = EM.endpoint_gaps(topo, labels, G, to)
                again = EM.endpoint_gaps(topo, labels, G, to)
                rows = EM.gap_table(topo, labels, gq, gd)
                e = _ms(lambda: EM.endpoint_gaps(topo, labels, G, to), a)
                e.update(gaps=int(rows.shape[0]), mutual=int(rows[:, 7].sum()), repeat_identical=bool(torch.equal(gq, again[0]) and torch.equal(gd, again[1])))
                r[f"endpoint_gaps_G{G}_{to}"] = e
        gq, gd = EM.endpoint_gaps(topo, labels, 16)
        groups = EM.gap_groups(labels, gq)
        r["groups_G16"] = int(EM._count_roots(groups).sum())
        r["gap_groups_G16"] = _ms(lambda: EM.gap_groups(labels, gq), a)
        r["gap_groups_repeat_identical"] = bool(torch.equal(groups, EM.gap_groups(labels, gq)))
        r["draw_bridges_G16"] = _ms(lambda: EM.draw_bridges(gq), a)
        r["bridge_px_G16"] = int((EM.draw_bridges(gq) * (sk == 0)).sum())
        r["gap_table_G16"] = _ms(lambda: EM.gap_table(topo, labels, gq, gd), a)
        r["skeleton_width_r64"] = _ms(lambda: EM.skeleton_width(x3, sk, t, 64), a)
        r["skeleton_topology"] = _ms(lambda: EM.skeleton_topology(sk), a)
        r["label_components"] = _ms(lambda: EM.label_components(x3, t), a)
        for G in GAPS:
            e = r[f"endpoint_gaps_G{G}_any"]
            e["over_skeleton_width_r64"] = round(e["ms"] / r["skeleton_width_r64"]["ms"], 3)
        if tag == "mask":
            gq64 = EM.endpoint_gaps(topo, labels, 64)[0]
            h = leg_host(topo[0], labels[0], gq64[0], 64)
            out["host_route_one_image"] = h
            e = r["endpoint_gaps_G64_any"]
            out["claim"] = {
                "search_8_images_G64_ms": e["ms"], "host_copy_one_image_ms": h["copy_ms"], "skeleton_width_r64_ms": r["skeleton_width_r64"]["ms"],
                "search_cheaper_than_the_host_copy_alone": bool(e["ms"] < h["copy_ms"]),
                "search_within_skeleton_width_at_the_same_radius": bool(e["ms"] <= r["skeleton_width_r64"]["ms"] * (1 + max(e["spread"] or 0, r["skeleton_width_r64"]["spread"] or 0)))}
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
    base = dict(measure_threshold=t, topology=True)
    modes = {"topology": base, "topology_bridge_16": dict(bridge_gap_px=16, **base), "topology_again": base}
    keys = ("skeleton_px", "endpoints", "n_gaps", "n_mutual_gaps", "bridge_px", "n_cracks_bridged", "max_gap_px")

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
    rate64, res64 = one_pass(dict(bridge_gap_px=64, **base))
    return {"images": a.images, "stitched": [4 * h, 4 * w], "passes": a.passes, "measure_threshold": round(t, 4),
            "set_fraction_image_0": round(float((first - t > 0).float().mean()), 5), "images_per_s": rates, "median": med, "spread": spread,
            "cost_of_bridging_16": round(1 - med["topology_bridge_16"] / med["topology"], 4),
            "same_configuration_twice": round(abs(1 - med["topology_again"] / med["topology"]), 4),
            "bridge_64_one_pass_images_per_s": round(rate64, 3), "image_0": {k: v[0] for k, v in last.items()}, "image_0_bridge_64": res64[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--legs", default="kernels,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaps_bench.json"))
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
