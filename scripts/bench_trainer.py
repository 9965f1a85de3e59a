"""Time the training driver (csbsr_amd/trainer.py) and the HIP SGD (csbsr_amd/optim.py) on the GPU.

    python scripts/bench_trainer.py                       # both legs, each in a child process under its own time limit
    python scripts/bench_trainer.py --leg overhead

Legs (one JSON line each; the parent prints them again as one JSON object and never opens the GPU itself):
  overhead  ms per step of the bare loop (zero_grad, forward, calc_loss, backward, optimizer.step) and of do_train(log_step=50), both fed by
            DeviceTrainLoader at HR 224 / batch 6 (the shipped yaml), two windows each, alternated.  Criterion: the trainer's mean is not
            above the bare loop's mean by more than the bare loop's own window-to-window spread.
  sgd       csbsr_amd.optim.SGD.step() against torch.optim.SGD.step() (momentum 0.9, weight decay 5e-4) on the full parameter set of the
            KBPN + PSPNet model: ms per step, kernel launches per step (torch.profiler), GB/s at 20 bytes per element (p, g and the buffer
            read, p and the buffer written).  Criterion: the HIP step is not slower.
Every window warms up first and is timed by the wall clock between two synchronisations, over >= 50 steps.
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


def make_dataset(hr, n, seed=0):
    rng = np.random.default_rng(seed)
    sizes = [(hr + int(rng.integers(0, 224)), hr + int(rng.integers(0, 224))) for _ in range(n)]
    images = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for H, W in sizes]
    masks = []
    for H, W in sizes:
        m = np.zeros((H, W), np.uint8)
        m[H // 2 - 3:H // 2 + 3, :] = 255
        m[:, W // 3:W // 3 + 5] = 255
        masks.append(m)
    return images, masks


def wall_ms(fn, n):
    """fn() once, covering n steps: wall ms per step between two synchronisations"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def leg_overhead(a):
    from csbsr_amd import trainer as T
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.resident import ResidentDataset, DeviceTrainLoader
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    ds = ResidentDataset(*make_dataset(a.hr, a.images), device=DEV)
    cfg = base_cfg.clone()
    cfg.SOLVER.BATCH_SIZE = a.batch
    torch.manual_seed(cfg.SEED)
    it0 = 40000
    model = JointModelWithLoss(cfg, len(ds), it0, None, device=DEV)
    model.train()
    opt = T.build_optimizer(cfg, model)
    loader = lambda n: DeviceTrainLoader(ds, a.hr, cfg.MODEL.SCALE_FACTOR, batch_size=a.batch, num_iterations=n, seed=1, drop_last=True)
    state = {"it": it0}

    def bare(n):
        for x, hr, mask, k, sdf in loader(n):
            state["it"] += 1
            opt.zero_grad()
            seg_l, sr_l = model(state["it"], x, sr_targets=hr, segment_targets=mask, kernel_targets=k, segment_sdf=sdf)[:2]
            T.calc_loss(seg_l, sr_l, state["it"], cfg).backward()
            opt.step()

    def driven(n):
        T.do_train(cfg, model, opt, T.build_scheduler(cfg, opt, state["it"]), loader(n), resume_iter=state["it"], log_step=a.steps,
                   log=lambda record: None)
        state["it"] += n
    bare(a.warmup)
    out = {"leg": "overhead", "hr": a.hr, "batch": a.batch, "steps": a.steps}
    for rep in range(2):                                 # alternate, so a drift of the machine shows up in both
        bare(2)
        out[f"bare_ms_{rep}"] = round(wall_ms(lambda: bare(a.steps), a.steps), 3)
        driven(2)
        out[f"trainer_ms_{rep}"] = round(wall_ms(lambda: driven(a.steps), a.steps), 3)
    b, t = (out["bare_ms_0"] + out["bare_ms_1"]) / 2, (out["trainer_ms_0"] + out["trainer_ms_1"]) / 2
    spread = abs(out["bare_ms_0"] - out["bare_ms_1"])
    out.update(bare_ms_mean=round(b, 3), trainer_ms_mean=round(t, 3), trainer_over_bare=round(t / b - 1, 4), bare_spread_ms=round(spread, 3),
               bare_spread=round(spread / b, 4), within_spread=bool(t - b <= spread), overflow_steps=int(model.overflow_steps))
    return out


def count_kernels(fn):
    """device kernel launches of one fn() call, from torch.profiler; None when the profiler reports no device events here"""
    from torch.profiler import profile, ProfilerActivity
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
            and "memset" not in e.name.lower())
    return n or None


def leg_sgd(a):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.optim import SGD
    model = JointModelWithLoss(base_cfg.clone(), 9000, 0, None, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    ph = [torch.nn.Parameter(p.detach().to(DEV).clone()) for p in model.parameters()]
    pt = [torch.nn.Parameter(p.detach().clone()) for p in ph]
    for x, y in zip(ph, pt):
        x.grad = torch.randn(x.shape, device=DEV, generator=gen) * 1e-3
        y.grad = x.grad.clone()
    n = sum(p.numel() for p in ph)
    hip = SGD(ph, lr=2e-5, momentum=0.9, weight_decay=5e-4)
    ref = torch.optim.SGD(pt, lr=2e-5, momentum=0.9, weight_decay=5e-4)
    steps = 4 * a.steps                                  # (a step is about a millisecond: a longer window than the other leg's)
    out = {"leg": "sgd", "tensors": len(ph), "elements": n, "steps": steps}

    def many(o, k):
        for _ in range(k):
            o.step()
    for o in (hip, ref):
        many(o, a.warmup)
    for rep in range(2):
        out[f"hip_ms_{rep}"] = round(wall_ms(lambda: many(hip, steps), steps), 4)
        out[f"torch_ms_{rep}"] = round(wall_ms(lambda: many(ref, steps), steps), 4)
    h, t = min(out["hip_ms_0"], out["hip_ms_1"]), min(out["torch_ms_0"], out["torch_ms_1"])
    err = max(float((x.detach() - y.detach()).abs().max() / y.detach().abs().max()) for x, y in zip(ph, pt))
    out.update(hip_ms=h, torch_ms=t, hip_gb_per_s=round(20 * n / h / 1e6, 1), torch_gb_per_s=round(20 * n / t / 1e6, 1),
               speedup=round(t / h, 3), not_slower=bool(h <= t), max_rel_diff_after_all_steps=err)
    try:
        out["hip_launches"], out["torch_launches"] = count_kernels(hip.step), count_kernels(ref.step)
    except Exception as e:                               # the timing above stands; the count is reported as missing, with the reason
        out["hip_launches"] = out["torch_launches"] = None
        out["launch_count_error"] = repr(e)[:200]
    return out


LEGS = {"overhead": leg_overhead, "sgd": leg_sgd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="one leg in this process (default: both, one child process each)")
    ap.add_argument("--hr", type=int, default=224)
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the collected JSON here")
    a = ap.parse_args()
    if a.steps < 50:
        ap.error("--steps must be at least 50")
    if a.leg:
        assert torch.cuda.is_available(), "this benchmark needs an MI355X"
        print(json.dumps(LEGS[a.leg](a)), flush=True)
        return
    results = []
    for leg in ("overhead", "sgd"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--hr", str(a.hr), "--batch", str(a.batch), "--images", str(a.images),
               "--steps", str(a.steps), "--warmup", str(a.warmup)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"leg {leg}: no result within {LEG_TIMEOUT_S} s; stopping", file=sys.stderr)
            sys.exit(124)
        if r.returncode != 0:                            # nothing more is started on the GPU after a failed leg
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            print(f"leg {leg} failed with status {r.returncode}; stopping", file=sys.stderr)
            sys.exit(r.returncode if r.returncode > 0 else 1)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    doc = json.dumps({"bench": "trainer", "legs": results})
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
