"""Time the MODEL.SR="bicubic" baseline on the GPU: the up-sampler against the one it sits next to, and the detector-only training step.

    python scripts/bench_bicubic_baseline.py                        # every leg, each in a child process under its own time limit
    python scripts/bench_bicubic_baseline.py --leg up               # one leg in this process

Legs (one JSON line each; the parent collects them into profiles/bicubic_baseline_bench.json and never opens the GPU itself):
  (a) up       csbsr_aa_bicubic_up (antialias 1, clip 0) at planes = 24, 448 x 448, x4 -- config 2's batch -- into a fresh output.
      up_add   csbsr_bicubic_up_add at the same shape (it reads the output back to add onto it).
      The two alternate, REPEATS children each; every child makes 5 warm-up and 50 timed calls between two events.  Criterion: the median
      of ``up`` is not above the median of ``up_add`` by more than the recorded spread (max - min) of the repeated legs.
  (b) step     at config 2's shapes (B = 8, LR 448 -> HR 1792, PSPNet, split precision, HIP Adam): img/s and ms per step of the
      detector-only step of the bicubic model, and beside it the joint step (KBPN + PSPNet) of the same process.  A record, no criterion.
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
LEG_TIMEOUT_S = {"up": 120, "up_add": 120, "step": 420}
REPEATS = 3
PLANES, LR, SCALE = 24, 448, 4


def leg_kernel(a):
    import ctypes as C
    from csbsr_amd import _lib as L
    P = lambda t: C.c_void_p(t.data_ptr())
    x = torch.rand(PLANES, LR, LR, device=DEV)
    y = torch.zeros(PLANES, LR * SCALE, LR * SCALE, device=DEV)
    st = L.stream(torch.device(DEV))
    if a.leg == "up":
        fn = lambda: L.call("csbsr_aa_bicubic_up", P(x), P(y), PLANES, LR, LR, SCALE, 1, 0, st)
    else:
        fn = lambda: L.call("csbsr_bicubic_up_add", P(x), P(y), PLANES, LR, LR, SCALE, st)
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.calls
    out_bytes = y.numel() * 4
    return {"leg": a.leg, "planes": PLANES, "lr": LR, "scale": SCALE, "calls": a.calls, "ms_event": round(ms, 4),
            "stored_GBps": round(out_bytes / ms / 1e6, 1)}


def leg_step(a):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.degrade import DeviceDegradation
    from csbsr_amd.data.synthetic import make_hr_mask
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.optim import Adam
    from csbsr_amd.trainer import calc_loss
    B, it = a.batch, 40000
    hr, mask = make_hr_mask(B, LR * SCALE, torch.Generator().manual_seed(1121))
    x, hr, mask, k, _ = DeviceDegradation(SCALE, device=DEV, seed=77)(hr, mask, with_sdf=False)
    x = x.clamp_(0, 1)
    out = {"leg": "step", "batch": B, "lr": LR, "scale": SCALE, "steps": a.steps, "warmup": a.step_warmup, "detector": "PSPNet",
           "detector_precision": "split"}
    for sr in ("bicubic", "KBPN"):
        cfg = base_cfg.clone()
        cfg.MODEL.SR = sr
        torch.manual_seed(cfg.SEED)
        model = JointModelWithLoss(cfg, 9000, it, None, device=DEV)
        model.micro_batch = 8
        model.train()
        model._runtime()
        opt = Adam([p for p in model.parameters() if p.requires_grad], lr=cfg.SOLVER.LR, betas=(0.9, 0.999), eps=1e-8)

        def step():
            opt.zero_grad(set_to_none=True)
            seg_l, sr_l = model(it, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)[:2]
            loss = calc_loss(seg_l, sr_l, it, cfg)
            loss.backward()
            opt.step()
            return loss
        for _ in range(a.step_warmup):
            step()
        torch.cuda.synchronize()
        ovf0, t0 = model.overflow_steps, time.perf_counter()
        for _ in range(a.steps):
            loss = step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if not bool(torch.isfinite(loss)) or model.overflow_steps != ovf0:
            raise SystemExit(f"{sr}: invalid timed region (loss {float(loss)}, overflowed steps {model.overflow_steps - ovf0})")
        key = "detector_only" if sr == "bicubic" else "joint"
        out[key] = {"imgs_per_s": round(B * a.steps / dt, 3), "ms_per_step": round(dt / a.steps * 1e3, 1), "loss": float(loss),
                    "peak_GB": round(torch.cuda.max_memory_allocated(DEV) / 1e9, 1)}
        del model, opt, step, loss
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(DEV)
    return out


def child(leg, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--calls", str(a.calls), "--warmup", str(a.warmup), "--steps", str(a.steps),
           "--step-warmup", str(a.step_warmup), "--batch", str(a.batch)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S[leg])
    except subprocess.TimeoutExpired:
        print(f"leg {leg}: no result within {LEG_TIMEOUT_S[leg]} s; stopping", file=sys.stderr)
        sys.exit(124)
    if r.returncode != 0:                                    # nothing more is started on the GPU after a failed leg
        print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
        print(f"leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
        sys.exit(r.returncode if r.returncode > 0 else 1)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("up", "up_add", "step"), default=None, help="one leg in this process (default: all, one child process each)")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--step-warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true", help="leg (a) only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicubic_baseline_bench.json"))
    a = ap.parse_args()
    if a.leg:
        assert torch.cuda.is_available(), "this benchmark needs an MI355X"
        print(json.dumps(leg_step(a) if a.leg == "step" else leg_kernel(a)), flush=True)
        return
    legs = []
    for _ in range(REPEATS):
        for leg in ("up", "up_add"):
            legs.append(child(leg, a))
    ms = {leg: [r["ms_event"] for r in legs if r["leg"] == leg] for leg in ("up", "up_add")}
    spread = max(max(v) - min(v) for v in ms.values())
    kernel = {"up_ms_median": float(np.median(ms["up"])), "up_add_ms_median": float(np.median(ms["up_add"])), "spread_ms": round(spread, 4),
              "up_not_slower_than_up_add": bool(np.median(ms["up"]) <= np.median(ms["up_add"]) + spread)}
    step = None if a.skip_step else child("step", a)
    doc = json.dumps({"bench": "bicubic_baseline", "kernel_legs": legs, "kernel": kernel, "step": step})
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
