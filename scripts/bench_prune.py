"""Time the spur pruning (csrc/prune.hip): estimate_metrics.prune_spurs at L = 4, 16 and 64 next to skeletonize and skeleton_topology on the
same masks in the same process, and predict_dataset with and without prune_spur_px=16.

    python scripts/bench_prune.py                         # writes profiles/prune_bench.json and prints it as one JSON line

  check    before anything is timed, prune_spurs on a small plane of synthetic cracks is asked for equality with the NumPy restatement of
           tests/prune_cases.py at L = 4, 16, 64 (out, T and the removed count).
  kernels  the 8 maps of 1792^2 of scripts/bench_skeleton.py: the sparse crack masks at 0.5 and the model-like maps at 0.01 (about 31 % set),
           skeletonised first.  Device events around ``reps`` calls after a warm-up, five such windows per call, the median reported with
           the spread (max / min - 1).  A prune_spurs call is the Python call: the scratch and output allocations, the two clears and the
           launches; csbsr_skeleton_prune alone is the entry on preallocated buffers.  A difference below the larger of two spreads is not
           a difference.
  dataset  predict_dataset without saving over synthetic LR images (stitched maps of 1792^2), config-2 model (deterministic fill): one
           warm-up pass each, then ``passes`` whole passes with measure_threshold + topology and with prune_spur_px=16 on top, alternating,
           the same with min_crack_px = 20."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_pr_sweep import DEV, crack_maps, windows  # noqa: E402

SPURS = (4, 16, 64)


def _ms(fn, a):
    med, spread, _ = windows(fn, a.reps, a.warmup)
    return {"ms": round(med, 4), "spread": round(spread, 4)}


def check():
    """the device against the restatement on the three synthetic crack skeletons of the tests (70 x 133)"""
    import prune_cases as PR
    from csbsr_amd.utils import estimate_metrics as EM
    planes = PR.cases()["cracks"]
    removed = {}
    for L in SPURS:
        out, rem, t = EM.prune_spurs(torch.from_numpy(planes).to(DEV), L, return_time=True)
        want = PR.prune_of(planes, L)
        assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(t.cpu().numpy(), want[1]) and np.array_equal(rem.cpu().numpy(), want[2]), L
        removed[str(L)] = rem.cpu().tolist()
    return {"planes": list(planes.shape), "equal_to_the_restatement": True, "removed": removed}


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
        r = {"set_fraction": round(float((x - t > 0).float().mean()), 5), "skeleton_px": int(sk.sum()),
             "endpoints": int(EM.skeleton_topology(sk)[1][:, 2].sum())}
        r["skeletonize"] = _ms(lambda: EM.skeletonize(x3, t), a)
        r["skeleton_topology"] = _ms(lambda: EM.skeleton_topology(sk), a)
        work = torch.empty(int(lib.csbsr_prune_work_bytes(N, H, W)), dtype=torch.uint8, device=sk.device)
        o2, t2, r2 = torch.empty_like(sk), torch.empty_like(sk), torch.empty(N, dtype=torch.int32, device=sk.device)
        for spur in SPURS:
            pruned, removed = EM.prune_spurs(sk, spur)
            again = EM.prune_spurs(sk, spur)
            e = _ms(lambda: EM.prune_spurs(sk, spur), a)
            e["entry_ms"] = _ms(lambda: L.call("csbsr_skeleton_prune", _ptr(sk), N, H, W, spur, _ptr(work), _ptr(t2), _ptr(o2), _ptr(r2),
                                               L.stream(sk.device)), a)
            e.update(repeat_identical=bool(torch.equal(pruned, again[0]) and torch.equal(removed, again[1])), removed_px=int(removed.sum()),
                     endpoints_left=int(EM.skeleton_topology(pruned)[1][:, 2].sum()),
                     over_skeletonize=round(e["ms"] / r["skeletonize"]["ms"], 2),
                     below_skeletonize_beyond_spread=bool(e["ms"] * (1 + max(e["spread"], r["skeletonize"]["spread"])) < r["skeletonize"]["ms"]))
            r[f"prune_spurs_{spur}"] = e
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
    modes = {"topology": dict(measure_threshold=t, topology=True), "topology_prune_16": dict(measure_threshold=t, topology=True, prune_spur_px=16),
             "min_crack_px_20_topology": dict(measure_threshold=t, min_crack_px=20, topology=True),
             "min_crack_px_20_topology_prune_16": dict(measure_threshold=t, min_crack_px=20, topology=True, prune_spur_px=16)}
    keys = ("crack_px", "skeleton_px", "spur_px", "n_cracks", "endpoints", "junctions", "loops", "length_geodesic_px", "mean_width_px")

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
    med = {k: float(np.median(v)) for k, v in rates.items()}
    return {"images": a.images, "stitched": [4 * h, 4 * w], "passes": a.passes, "measure_threshold": round(t, 4),
            "set_fraction_image_0": round(float((first - t > 0).float().mean()), 5), "images_per_s": rates, "median": med,
            "spread": {k: round(max(v) / min(v) - 1, 4) for k, v in rates.items()},
            "cost_of_prune_16": {"topology": round(1 - med["topology_prune_16"] / med["topology"], 4),
                                 "min_crack_px_20_topology": round(1 - med["min_crack_px_20_topology_prune_16"] / med["min_crack_px_20_topology"], 4)},
            "image_0": {k: v[0] for k, v in last.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=1792)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--legs", default="kernels,dataset")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_bench.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "check": check()}
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
