"""Time the scale-jittered crop of the HBM-resident loader (csbsr_gather_resize_u8, csbsr_amd/data/resident.py) on the GPU.

    python scripts/bench_resized_crop.py                            # every leg below, each in a child process under its own time limit
    python scripts/bench_resized_crop.py --leg fused --hr 224 --batch 6

Legs (one JSON line each; the parent prints them again as one JSON object and never opens the GPU itself), at the shipped yaml's size
(HR 224, batch 6) and the benchmark's (HR 1792, batch 8), scale (0.5, 1.0), ratio (3/4, 4/3), the same window tables for every leg:
  fused   ResidentDataset.gather_resized: hr and mask of a batch in two launches.
  chain   what a user could write without the kernel: per sample, csbsr_gather_crop_u8 of the window at its own size (image and mask),
          then torch.nn.functional.interpolate(mode="bilinear", antialias=True) on the device, written into the batch tensors.
  plain   csbsr_gather_crop_u8 alone at the same output size (no resample): the floor.
Every leg runs 5 warm-up and 50 timed batches per window between two synchronisations, five windows; it reports the median window and
the spread (max - min) of its windows, event time and wall time per batch.  Criterion: fused <= chain + the chain's own spread.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
LEG_TIMEOUT_S = 420
WINDOWS = 5
RESIZED = {"scale": (0.5, 1.0), "ratio": (0.75, 4 / 3)}


def make_dataset(hr, n, seed=0):
    """n uint8 image / mask pairs around the crop size and up to twice it per side, of mixed sizes"""
    rng = np.random.default_rng(seed)
    sizes = [(hr + int(rng.integers(0, hr)), hr + int(rng.integers(0, hr))) for _ in range(n)]
    images = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for H, W in sizes]
    masks = []
    for H, W in sizes:
        m = np.zeros((H, W), np.uint8)
        m[H // 2 - 3:H // 2 + 3, :] = 255
        m[:, W // 3:W // 3 + 5] = 255
        masks.append(m)
    return images, masks


def timed(fn, n, warmup):
    """fn() n times after `warmup` calls: (event ms per call, wall ms per call), both between two synchronisations."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, (time.perf_counter() - t0) * 1e3 / n


def windows(fn, a):
    ev, wall = zip(*[timed(fn, a.batches, a.warmup) for _ in range(WINDOWS)])
    return {"ms_event_median": round(float(np.median(ev)), 4), "ms_event_spread": round(max(ev) - min(ev), 4),
            "ms_wall_median": round(float(np.median(wall)), 4), "ms_wall_spread": round(max(wall) - min(wall), 4)}


def setup(a):
    from csbsr_amd.data.resident import ResidentDataset, DeviceTrainLoader
    images, masks = make_dataset(a.hr, a.images)
    ds = ResidentDataset(images, masks, device=DEV)
    ld = DeviceTrainLoader(ds, a.hr, 4, batch_size=a.batch, seed=1, drop_last=True, resized_crop=RESIZED)
    tables = [ld.draw()[0] for _ in range(8)]               # the same tables in every leg (one seed), cycled
    for t in tables:
        assert t.shape == (a.batch, 7), "the pool must hold a multiple of the batch size (no short batch at the end of an epoch)"
        ds.check_windows(t.numpy(), a.hr, a.hr)
    return ds, tables


def leg_fused(a):
    ds, tables = setup(a)
    dev = [t.to(DEV) for t in tables]
    state = {"i": 0}

    def fn():
        state["i"] += 1
        return ds.gather_resized(dev[state["i"] % len(dev)], a.batch, a.hr, a.hr, True)
    return {"leg": "fused", "hr": a.hr, "batch": a.batch, "batches": a.batches, **windows(fn, a)}


def leg_chain(a):
    import torch.nn.functional as F
    ds, tables = setup(a)
    # per sample one [1,5] row of the plain gather on the device, made once: the chain is not charged for its table uploads
    rows = [[(t[s:s + 1, :5].contiguous().to(DEV), int(t[s, 5]), int(t[s, 6])) for s in range(a.batch)] for t in tables]
    hr = torch.empty(a.batch, 3, a.hr, a.hr, device=DEV)
    mask = torch.empty(a.batch, 1, a.hr, a.hr, device=DEV)
    state = {"i": 0}

    def fn():
        state["i"] += 1
        for s, (row, hs, ws) in enumerate(rows[state["i"] % len(rows)]):
            wi, wm = ds.gather(row, 1, hs, ws)
            hr[s:s + 1] = F.interpolate(wi, size=(a.hr, a.hr), mode="bilinear", align_corners=False, antialias=True)
            mask[s:s + 1] = F.interpolate(wm, size=(a.hr, a.hr), mode="bilinear", align_corners=False, antialias=True)
        return hr, mask
    out = {"leg": "chain", "hr": a.hr, "batch": a.batch, "batches": a.batches, **windows(fn, a)}
    # the two paths compute the same thing (torch's device kernel rounds differently: a figure, not an assertion)
    state["i"] = 0
    got = [t.clone() for t in fn()]
    want = ds.gather_resized(tables[1].to(DEV), a.batch, a.hr, a.hr, True)
    out["max_abs_diff_to_fused"] = float(max((g - w).abs().max() for g, w in zip(got, want)))
    return out


def leg_plain(a):
    from csbsr_amd.data.resident import DeviceTrainLoader
    ds, _ = setup(a)
    ld = DeviceTrainLoader(ds, a.hr, 4, batch_size=a.batch, seed=1, drop_last=True)
    dev = [ld.draw()[0].to(DEV) for _ in range(8)]
    assert all(t.shape == (a.batch, 5) for t in dev)
    state = {"i": 0}

    def fn():
        state["i"] += 1
        return ds.gather(dev[state["i"] % len(dev)], a.batch, a.hr, a.hr)
    return {"leg": "plain", "hr": a.hr, "batch": a.batch, "batches": a.batches, **windows(fn, a)}


LEGS = {"fused": leg_fused, "chain": leg_chain, "plain": leg_plain}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="one leg in this process (default: all legs, one child process each)")
    ap.add_argument("--hr", type=int, default=224)
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--images", type=int, default=0, help="images in the pool, a multiple of the batch size (0: 96 at HR <= 448, else 16)")
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the collected JSON here")
    a = ap.parse_args()
    if a.batches < 50:
        ap.error("--batches must be at least 50")
    if a.leg:
        a.images = a.images or (96 if a.hr <= 448 else 16)
        assert torch.cuda.is_available(), "this benchmark needs an MI355X"
        print(json.dumps(LEGS[a.leg](a)), flush=True)
        return
    results = []
    for hr, batch in ((224, 6), (1792, 8)):
        for leg in ("fused", "chain", "plain"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--hr", str(hr), "--batch", str(batch), "--batches", str(a.batches),
                   "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                print(f"leg {leg} hr {hr}: no result within {LEG_TIMEOUT_S} s; stopping", file=sys.stderr)
                sys.exit(124)
            if r.returncode != 0:                            # nothing more is started on the GPU after a failed leg
                print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                print(f"leg {leg} hr {hr} failed with status {r.returncode}; stopping", file=sys.stderr)
                sys.exit(r.returncode if r.returncode > 0 else 1)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            results.append(json.loads(line))
    by = {(r["leg"], r["hr"]): r for r in results}
    verdict = {str(hr): bool(by[("fused", hr)]["ms_event_median"] <= by[("chain", hr)]["ms_event_median"] + by[("chain", hr)]["ms_event_spread"])
               for hr in (224, 1792)}
    doc = json.dumps({"bench": "resized_crop", "legs": results, "fused_not_slower_than_chain": verdict})
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
