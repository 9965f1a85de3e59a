"""Time one SR-only pretraining step (SRModelWithLoss) next to the step that trained KBPN alone before it existed: a
JointModelWithLoss(PSPNet) at an iteration inside SR_PRETRAIN_ITER with ``loss = sr_loss.mean()``.

    python scripts/bench_pretrain_sr.py --out profiles/pretrain_sr_bench.json

One process, both models alive in it, the same batch for both.  A step is zero_grad, forward, ``sr_loss.mean().backward()`` and the HIP Adam
step.  Per shape every model first runs ``--warmup`` steps (code objects, allocator, slope probes), then the two are timed in turn,
``--rounds`` times over -- so a drift of the machine shows up in both and the spread of repeated identical windows stands beside the
difference --, each window ``--steps`` steps between two device synchronisations on the host clock.  Peak memory is torch's
max_memory_allocated over a timed window; ``resident`` is the number of KBPN micro-batches that kept their activations for the backward
(the others are recomputed there), with the micro-batch the model chose.

Shapes: config 2's (B = 8, LR 448 -> HR 1792) and a pretraining patch shape (B = 16, LR 64 -> HR 256).  Inputs: synthetic HR textures
degraded on the device (csbsr_amd.data.degrade), seeded.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
IT = 20001          # inside SR_PRETRAIN_ITER [1, 30001), past both KBPN module-pretraining windows: every KBPN tensor trains
SHAPES = {"config2": (8, 448), "patch": (16, 64)}


def make_models(cfg):
    from csbsr_amd import trainer as T
    from csbsr_amd.modeling.build_model import JointModelWithLoss, SRModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    out = {}
    for name, m in (("sr_only", SRModelWithLoss(cfg, device=DEV)), ("joint_sr_phase", JointModelWithLoss(cfg, 1000, 0, None, device=DEV))):
        deterministic_fill(m.state_dict(), "contractive")
        m.train()
        m._runtime()
        out[name] = (m, T.build_optimizer(cfg, m))
    return out


def make_batch(B, lr, scale, seed):
    from csbsr_amd.data.degrade import DeviceDegradation
    from csbsr_amd.data.synthetic import make_hr_mask
    hr, mask = make_hr_mask(B, lr * scale, torch.Generator().manual_seed(seed))
    return DeviceDegradation(scale, device=DEV, seed=seed)(hr, mask)          # (x, hr, mask, k, sdf) on the device


def step(name, model, opt, batch):
    x, hr, mask, k, sdf = batch
    opt.zero_grad()
    if name == "sr_only":
        sr_l = model(IT, x, sr_targets=hr, kernel_targets=k)[0]
    else:
        sr_l = model(IT, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, segment_sdf=sdf)[1]
    sr_l.mean().backward()
    opt.step()


def window(name, model, opt, batch, steps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    t0 = time.perf_counter()
    for _ in range(steps):
        step(name, model, opt, batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, torch.cuda.max_memory_allocated(DEV)


def bench_shape(label, B, lr, cfg, a):
    models = make_models(cfg)
    batch = make_batch(B, lr, cfg.MODEL.SCALE_FACTOR, seed=3)
    steps = a.steps if label == "config2" else a.patch_steps
    for name, (m, opt) in models.items():
        for _ in range(a.warmup):
            step(name, m, opt, batch)
        assert not m.last_step_overflowed, name
    torch.cuda.synchronize()
    t, peak = {n: [] for n in models}, {n: 0 for n in models}
    for _ in range(a.rounds):
        for name, (m, opt) in models.items():
            dt, pk = window(name, m, opt, batch, steps)
            t[name].append(dt)
            peak[name] = max(peak[name], pk)
    rows = {}
    for name, (m, _) in models.items():
        best = min(t[name])
        n_mb = -(-B // m._mb_used)
        rows[name] = {"ms_per_step": [round(v * 1e3, 2) for v in t[name]], "ms_per_step_best": round(best * 1e3, 2),
                      "img_per_s_best": round(B / best, 3), "spread": round(max(t[name]) / best - 1, 4),
                      "peak_memory_GB": round(peak[name] / 1e9, 2), "micro_batch": int(m._mb_used), "micro_batches": int(n_mb),
                      "resident_micro_batches": int(min(m._n_res, n_mb)), "lean_saves": bool(m._lean), "overflow_steps": int(m.overflow_steps)}
    sr, jo = rows["sr_only"], rows["joint_sr_phase"]
    noise = max(sr["spread"], jo["spread"])
    out = {"shape": label, "B": B, "lr": lr, "hr": lr * cfg.MODEL.SCALE_FACTOR, "iteration": IT, "steps_per_window": steps, "rounds": a.rounds,
           "warmup_steps": a.warmup, **rows, "sr_only_over_joint_time": round(sr["ms_per_step_best"] / jo["ms_per_step_best"], 4),
           "sr_only_not_slower": bool(sr["ms_per_step_best"] <= jo["ms_per_step_best"] * (1 + noise)),
           "sr_only_more_resident": bool(sr["resident_micro_batches"] * sr["micro_batch"] > jo["resident_micro_batches"] * jo["micro_batch"])}
    del models, batch
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=sorted(SHAPES), default=["patch", "config2"])
    ap.add_argument("--steps", type=int, default=3, help="steps per timed window at config 2's shape (seconds each)")
    ap.add_argument("--patch-steps", type=int, default=20, help="steps per timed window at the patch shape")
    ap.add_argument("--rounds", type=int, default=3, help="times the pair of windows is repeated")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_sr_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    from csbsr_amd.config import cfg as base_cfg
    results = []
    for label in a.shapes:
        cfg = base_cfg.clone()
        cfg.SOLVER.BATCH_SIZE = SHAPES[label][0]
        r = bench_shape(label, *SHAPES[label], cfg, a)
        print(json.dumps(r), flush=True)
        results.append(r)
    doc = {"bench": "pretrain_sr", "device": torch.cuda.get_device_name(0), "shapes": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
