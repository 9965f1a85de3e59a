"""Time csbsr_area_down_fwd / _bwd next to csbsr_aa_bicubic_down_fwd / _bwd, and one train step with SOLVER.DOWNSCALE_INTERPOLATION = 'area'
next to the same step with 'bicubic'.

    python scripts/bench_area_down.py --out profiles/area_down_bench.json

Kernels: planes 24 x 1792^2 (the config-2 loss: B = 8, three channels) and planes 48 x 256^2 (a patch batch), both at f = 4.  Per shape
every kernel is warmed, then the four are timed in turn, ``--rounds`` times over, each window as many launches as fill ``--window-s``
seconds (counted from a first timed launch) between two device events.  Successive launches rotate over buffer sets that together
exceed the last-level cache (``--rotate-mb``), so the rate is that of memory, not of a cache that happens to hold the last input.  GB/s comes from the algorithmic bytes: the full-resolution
planes once plus the low-resolution planes once (the backward runs with accumulate = 0 and reads no dx).  ``spread`` is max / min - 1
over the rounds of identical windows; a difference between two kernels below the larger of their spreads is not a difference.

Step: JointModelWithLoss(PSPNet) at config 2's shape (B = 8, LR 448 -> HR 1792), joint phase, zero_grad + forward + calc_loss + backward +
HIP Adam; both models alive in the process, each fed a batch degraded with its own down-scale, timed in turn between host-side
synchronisations."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
IT = 40000
KERNEL_SHAPES = {"config2_loss": (24, 1792, 1792, 4), "patch_batch": (48, 256, 256, 4)}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def kernel_calls(planes, H, W, f, sets):
    """the four launches, each call on the next of ``sets`` buffer sets: together they exceed the 256 MB last-level cache, so a launch
    finds none of its input there (one set launched over and over reads part of its 308 MB from that cache)"""
    from csbsr_amd import _lib as L
    bufs = [(torch.rand(planes, H, W, device=DEV), torch.rand(planes, H // f, W // f, device=DEV)) for _ in range(sets)]
    bufs = [(big, small, torch.empty_like(big), torch.empty_like(small)) for big, small in bufs]
    st = L.stream(torch.device(DEV))
    turn = [0]

    def on_next(fn):
        def call():
            turn[0] = (turn[0] + 1) % sets
            fn(*bufs[turn[0]])
        return call
    return {
        "area_fwd": on_next(lambda big, small, big_out, small_out: L.call("csbsr_area_down_fwd", _ptr(big), _ptr(small_out), planes, H, W, f, st)),
        "bicubic_fwd": on_next(lambda big, small, big_out, small_out: L.call("csbsr_aa_bicubic_down_fwd", _ptr(big), _ptr(small_out), planes, H, W, f, 1, st)),
        "area_bwd": on_next(lambda big, small, big_out, small_out: L.call("csbsr_area_down_bwd", _ptr(small), _ptr(big_out), 0, planes, H, W, f, st)),
        "bicubic_bwd": on_next(lambda big, small, big_out, small_out: L.call("csbsr_aa_bicubic_down_bwd", _ptr(small), _ptr(big_out), 0, planes, H, W, f, 1, st)),
    }, bufs


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def bench_kernels(label, shape, a):
    planes, H, W, f = shape
    nbytes = 4 * planes * (H * W + (H // f) * (W // f))
    sets = max(2, -(-a.rotate_mb * 1000000 // (4 * planes * H * W)))          # full-resolution planes of all sets together >= --rotate-mb
    calls, keep = kernel_calls(*shape, sets)
    reps = {}
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        reps[name] = max(5, int(a.window_s * 1e3 / max(timed(fn, 3), 1e-3)) + 1)
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms[name].append(timed(fn, reps[name]))
    rows = {name: {"ms": [round(v, 4) for v in t], "ms_best": round(min(t), 4), "GB_per_s_best": round(nbytes / min(t) / 1e6, 1),
                   "spread": round(max(t) / min(t) - 1, 4), "launches_per_window": reps[name]} for name, t in ms.items()}
    out = {"shape": label, "planes": planes, "H": H, "W": W, "f": f, "algorithmic_MB": round(nbytes / 1e6, 1), "rounds": a.rounds, "buffer_sets": sets, **rows}
    for d in ("fwd", "bwd"):
        ar, bi = rows["area_" + d], rows["bicubic_" + d]
        out[f"area_over_bicubic_{d}"] = round(ar["ms_best"] / bi["ms_best"], 4)
        out[f"area_not_slower_{d}"] = bool(ar["ms_best"] <= bi["ms_best"] * (1 + max(ar["spread"], bi["spread"])))
    del calls, keep
    torch.cuda.empty_cache()
    return out


def bench_step(a):
    from csbsr_amd import trainer as T
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.degrade import DeviceDegradation
    from csbsr_amd.data.synthetic import make_hr_mask
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    B, lr = a.batch, a.lr_size
    hr, mask = make_hr_mask(B, lr * 4, torch.Generator().manual_seed(3))
    runs = {}
    for mode in ("area", "bicubic"):
        cfg = base_cfg.clone()
        cfg.SOLVER.BATCH_SIZE, cfg.SOLVER.DOWNSCALE_INTERPOLATION = B, mode
        m = JointModelWithLoss(cfg, 1000, 0, None, device=DEV)
        deterministic_fill(m.state_dict(), "contractive")
        m.train()
        m._runtime()
        batch = DeviceDegradation(4, device=DEV, seed=3, interpolation=mode)(hr, mask)
        runs[mode] = (cfg, m, T.build_optimizer(cfg, m), batch)

    def step(mode):
        cfg, m, opt, (x, hr_d, mask_d, k, sdf) = runs[mode]
        opt.zero_grad()
        seg_l, sr_l = m(IT, x, sr_targets=hr_d, segment_targets=mask_d, kernel_targets=k, segment_sdf=sdf)[:2]
        T.calc_loss(seg_l, sr_l, IT, cfg).backward()
        opt.step()
    for mode in runs:
        for _ in range(a.warmup):
            step(mode)
        assert not runs[mode][1].last_step_overflowed, mode
    t = {mode: [] for mode in runs}
    for _ in range(a.step_rounds):
        for mode in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(mode)
            torch.cuda.synchronize()
            t[mode].append((time.perf_counter() - t0) / a.steps)
    rows = {mode: {"ms_per_step": [round(v * 1e3, 2) for v in ts], "ms_per_step_best": round(min(ts) * 1e3, 2),
                   "img_per_s_best": round(B / min(ts), 3), "spread": round(max(ts) / min(ts) - 1, 4)} for mode, ts in t.items()}
    noise = max(r["spread"] for r in rows.values())
    return {"B": B, "lr": lr, "hr": lr * 4, "iteration": IT, "steps_per_window": a.steps, "rounds": a.step_rounds, "warmup_steps": a.warmup, **rows,
            "area_over_bicubic_step": round(rows["area"]["ms_per_step_best"] / rows["bicubic"]["ms_per_step_best"], 4),
            "area_not_slower": bool(rows["area"]["ms_per_step_best"] <= rows["bicubic"]["ms_per_step_best"] * (1 + noise))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=0.5, help="seconds of launches per timed kernel window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rotate-mb", type=int, default=1200, help="the launches of a window rotate over buffer sets of at least this many MB")
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--lr-size", type=int, default=448)
    ap.add_argument("--steps", type=int, default=2, help="steps per timed window of the train step")
    ap.add_argument("--step-rounds", type=int, default=3, help="times the pair of train-step windows is repeated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "area_down_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    from csbsr_amd.engine import Engine
    eng = Engine(torch.device(DEV))          # registers the reduction scratch csbsr_aa_bicubic_down_bwd keeps its weight tables in
    doc = {"bench": "area_down", "device": torch.cuda.get_device_name(0), "kernels": []}
    for label, shape in KERNEL_SHAPES.items():
        r = bench_kernels(label, shape, a)
        print(json.dumps(r), flush=True)
        doc["kernels"].append(r)
    if not a.no_step:
        doc["train_step"] = bench_step(a)
        print(json.dumps(doc["train_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
