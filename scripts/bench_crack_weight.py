"""Time csbsr_crack_weight (the crack-oriented SR-loss weight, SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP) next to csbsr_sdf on the same masks,
and one train step with the key next to the same step without it.

    python scripts/bench_crack_weight.py --out profiles/crack_weight_bench.json

Kernels: 8 masks of 1792^2 (the config-2 loss shape), the sparse crack masks bench.py trains on (csbsr_amd.data.synthetic.make_hr_mask at
full size: no tiling of a small batch, whose periodic cracks would keep the row pass's search short), amp 0.1, LR map at s = 4.  Both entry
points are warmed, then timed in turn ``--rounds`` times over, each window as many calls as fill ``--window-s`` seconds between two device
events.  ``spread`` is max / min - 1 over the rounds of identical windows; a difference below the larger of two spreads is not a difference.
csbsr_sdf runs the exact transform twice (inside and outside distance) plus a combine pass, csbsr_crack_weight once with the exponential
in the row pass; both search times depend on the masks, so the ratio holds for these masks only.

Step: JointModelWithLoss(PSPNet) at config 2's shape (B = 8, LR 448 -> HR 1792), iteration 40000, zero_grad + forward + calc_loss +
backward + HIP Adam; a model with CRACK_ORIENTED_WEIGHT4SR_AMP = 0.1 / ORIENTED_WEIGHT_ITER = 0 and one without live in the process, fed
the same batch and timed in turn between host-side synchronisations."""
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


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def bench_kernels(a):
    from csbsr_amd import _lib as L
    from csbsr_amd.data.synthetic import make_hr_mask
    N, H, s = a.batch, a.lr_size * 4, 4
    mask = make_hr_mask(N, H, torch.Generator().manual_seed(3))[1].to(DEV).contiguous()
    w_hr, w_lr, sdf = torch.empty_like(mask), torch.empty(N, 1, H // s, H // s, device=DEV), torch.empty_like(mask)
    scratch = torch.empty(3 * N * H * H + 2 * N, device=DEV)
    st = L.stream(torch.device(DEV))
    calls = {
        "crack_weight": lambda: L.call("csbsr_crack_weight", _ptr(mask), _ptr(w_hr), _ptr(w_lr), _ptr(scratch), N, H, H, 0.1, 2.0, s, st),
        "crack_weight_hr_only": lambda: L.call("csbsr_crack_weight", _ptr(mask), _ptr(w_hr), None, _ptr(scratch), N, H, H, 0.1, 2.0, s, st),
        "sdf": lambda: L.call("csbsr_sdf", _ptr(mask), _ptr(sdf), _ptr(scratch), N, H, H, st),
    }
    reps = {}
    for name, fn in calls.items():
        for _ in range(3):
            fn()
        reps[name] = max(5, int(a.window_s * 1e3 / max(timed(fn, 3), 1e-3)) + 1)
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms[name].append(timed(fn, reps[name]))
    rows = {name: {"ms": [round(v, 4) for v in t], "ms_best": round(min(t), 4), "spread": round(max(t) / min(t) - 1, 4),
                   "calls_per_window": reps[name]} for name, t in ms.items()}
    # bytes the three launches must move: mask read + g written, re-read and re-written by the column pass, g read + w_hr written by the
    # row pass, w_hr read + w_lr written by the reduction
    px = N * H * H
    nbytes = 4 * (px * 4 + px * 2 + px + px // (s * s))
    rows["crack_weight"]["GB_per_s_best"] = round(nbytes / rows["crack_weight"]["ms_best"] / 1e6, 1)
    return {"N": N, "H": H, "W": H, "scale": s, "amp": 0.1, "foreground_fraction": round(float(mask.mean()), 5), "rounds": a.rounds,
            "algorithmic_MB": round(nbytes / 1e6, 1), **rows,
            "crack_weight_over_sdf": round(rows["crack_weight"]["ms_best"] / rows["sdf"]["ms_best"], 4)}


def bench_step(a):
    from csbsr_amd import trainer as T
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.degrade import DeviceDegradation
    from csbsr_amd.data.synthetic import make_hr_mask
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    B, lr = a.batch, a.lr_size
    hr, mask = make_hr_mask(B, lr * 4, torch.Generator().manual_seed(3))
    batch = DeviceDegradation(4, device=DEV, seed=3)(hr, mask)
    runs = {}
    for mode, amp in (("crack_weight", 0.1), ("plain", 0.0)):
        cfg = base_cfg.clone()
        cfg.SOLVER.BATCH_SIZE, cfg.SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP, cfg.SOLVER.ORIENTED_WEIGHT_ITER = B, amp, 0
        m = JointModelWithLoss(cfg, 1000, 0, None, device=DEV)
        deterministic_fill(m.state_dict(), "contractive")
        m.train()
        m._runtime()
        runs[mode] = (cfg, m, T.build_optimizer(cfg, m))

    def step(mode):
        cfg, m, opt = runs[mode]
        x, hr_d, mask_d, k, sdf = batch
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
    return {"B": B, "lr": lr, "hr": lr * 4, "iteration": IT, "steps_per_window": a.steps, "rounds": a.step_rounds, "warmup_steps": a.warmup, **rows,
            "crack_weight_minus_plain_ms": round(rows["crack_weight"]["ms_per_step_best"] - rows["plain"]["ms_per_step_best"], 2),
            "noise_ms": round(max(r["spread"] * r["ms_per_step_best"] for r in rows.values()), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-s", type=float, default=0.5, help="seconds of calls per timed kernel window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--lr-size", type=int, default=448)
    ap.add_argument("--steps", type=int, default=2, help="steps per timed window of the train step")
    ap.add_argument("--step-rounds", type=int, default=3, help="times the pair of train-step windows is repeated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crack_weight_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    doc = {"bench": "crack_weight", "device": torch.cuda.get_device_name(0)}
    doc["kernels"] = bench_kernels(a)
    print(json.dumps(doc["kernels"]), flush=True)
    torch.cuda.empty_cache()
    if not a.no_step:
        doc["train_step"] = bench_step(a)
        print(json.dumps(doc["train_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
