"""Time the HBM-resident training loader (csbsr_amd/data/resident.py) on the GPU.

    python scripts/bench_resident_loader.py                         # every leg below, each in a child process under its own time limit
    python scripts/bench_resident_loader.py --leg loader --hr 224 --batch 6

Legs (one JSON line each; the parent prints them again as one JSON object and never opens the GPU itself):
  loader  batches per second of DeviceTrainLoader alone, next to the same batches -- the same decision tables -- made the way the code
          before this loader had to make them: host uint8 -> numpy flip / crop -> fp32 / 255 -> DeviceDegradation.__call__ with its
          host-to-device copy inside.  Sizes: the shipped yaml's (HR 224, batch 6) and the benchmark's (HR 1792, batch 8).
  kernel  csbsr_gather_crop_u8 alone: effective bytes per second (source bytes read + fp32 bytes written, over the event time) next to a
          device-to-device copy of the same output bytes, and the ratio of the two times.
  step    one training step (forward, losses, backward, Adam) at HR 224 / batch 6 fed by the loader against the same step fed one fixed
          resident batch: the loader's share of a step.
Every leg warms up first and times with events over >= 50 batches; the wall clock between two synchronisations is printed beside them.
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
    """n uint8 image / mask pairs somewhat larger than the crop, of mixed sizes (448^2-like for HR 224)."""
    rng = np.random.default_rng(seed)
    pad = max(8, hr // 8) if hr > 448 else 224
    sizes = [(hr + int(rng.integers(0, pad)), hr + int(rng.integers(0, pad))) for _ in range(n)]
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


def host_batch(images, masks, sel, h, w):
    """The batch the way the host had to make it: numpy flips and crop per sample, then fp32 / 255."""
    hr, mk = [], []
    for idx, y0, x0, mirror, vflip in sel.tolist():
        a, m = images[idx], masks[idx][:, :, None]
        if mirror:
            a, m = a[:, ::-1], m[:, ::-1]
        if vflip:
            a, m = a[::-1], m[::-1]
        hr.append(a[y0:y0 + h, x0:x0 + w].astype(np.float32).transpose(2, 0, 1))
        mk.append(m[y0:y0 + h, x0:x0 + w].astype(np.float32).transpose(2, 0, 1))
    return torch.from_numpy(np.stack(hr)) / 255, torch.from_numpy(np.stack(mk)) / 255


def leg_loader(a):
    from csbsr_amd.data.degrade import DeviceDegradation
    from csbsr_amd.data.resident import ResidentDataset, DeviceTrainLoader
    images, masks = make_dataset(a.hr, a.images)
    ds = ResidentDataset(images, masks, device=DEV)
    ld = DeviceTrainLoader(ds, a.hr, 4, batch_size=a.batch, num_iterations=a.warmup + a.batches, seed=1, drop_last=True)
    tables = list(ld.iter_decisions())
    # the new path: decisions drawn inside the timed loop, as a training run does
    ld2 = DeviceTrainLoader(ds, a.hr, 4, batch_size=a.batch, seed=1, drop_last=True)
    new_ev, new_wall = timed(lambda: ld2.batch(*ld2.draw()), a.batches, a.warmup)
    deg = DeviceDegradation(4, device=DEV)
    it = iter(tables)

    def old():
        sel, params = next(it)
        deg(*host_batch(images, masks, sel.numpy(), a.hr, a.hr), params=params)
    old_ev, old_wall = timed(old, a.batches, a.warmup)
    # same tables -> same tensors (the host path's `/ 255` is torch's, the comparison the tests make bit for bit)
    sel, params = tables[0]
    got, want = ld.batch(sel, params), deg(*host_batch(images, masks, sel.numpy(), a.hr, a.hr), params=params)
    same = all(torch.equal(g, w) for g, w in zip(got, want))
    return {"leg": "loader", "hr": a.hr, "batch": a.batch, "batches": a.batches, "pool_mb": round(ds.nbytes / 2**20, 1),
            "resident_ms_event": round(new_ev, 4), "resident_ms_wall": round(new_wall, 4), "resident_batches_per_s": round(1e3 / new_wall, 1),
            "host_path_ms_event": round(old_ev, 4), "host_path_ms_wall": round(old_wall, 4), "host_path_batches_per_s": round(1e3 / old_wall, 1),
            "speedup_wall": round(old_wall / new_wall, 2), "outputs_identical": bool(same)}


def leg_kernel(a):
    from csbsr_amd.data.resident import ResidentDataset, DeviceTrainLoader
    images, masks = make_dataset(a.hr, a.images)
    ds = ResidentDataset(images, masks, device=DEV)
    ld = DeviceTrainLoader(ds, a.hr, 4, batch_size=a.batch, seed=1, drop_last=True)
    sel = ld.draw()[0].to(DEV)
    B, h = a.batch, a.hr
    hr, mask = ds.gather(sel, B, h, h)
    both, _ = timed(lambda: ds.gather(sel, B, h, h), a.batches, a.warmup)
    dst_i, dst_m = torch.empty_like(hr), torch.empty_like(mask)

    def copy():
        dst_i.copy_(hr)
        dst_m.copy_(mask)
    cp, _ = timed(copy, a.batches, a.warmup)
    out_bytes = 4 * B * 4 * h * h                       # fp32, 3 + 1 planes
    moved = out_bytes + out_bytes // 4                  # + the uint8 source
    return {"leg": "kernel", "hr": a.hr, "batch": a.batch, "reps": a.batches, "gather_ms": round(both, 4), "gather_bytes": moved,
            "gather_gb_per_s": round(moved / both / 1e6, 1), "d2d_copy_ms": round(cp, 4), "d2d_copy_bytes": 2 * out_bytes,
            "d2d_copy_gb_per_s": round(2 * out_bytes / cp / 1e6, 1), "gather_over_copy_time": round(both / cp, 3)}


def leg_step(a):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.resident import ResidentDataset, DeviceTrainLoader
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.optim import Adam
    images, masks = make_dataset(a.hr, a.images)
    ds = ResidentDataset(images, masks, device=DEV)
    ld = DeviceTrainLoader(ds, a.hr, 4, batch_size=a.batch, seed=1, drop_last=True)
    cfg = base_cfg.clone()
    torch.manual_seed(cfg.SEED)
    model = JointModelWithLoss(cfg, 9000, 40000, None, device=DEV)
    model.train()
    opt = Adam([p for p in model.parameters() if p.requires_grad], lr=cfg.SOLVER.LR, betas=(0.9, 0.999), eps=1e-8)
    beta = cfg.SOLVER.TASK_LOSS_WEIGHT
    fixed = ld.batch(*ld.draw())

    def step(batch):
        x, hr, mask, k, sdf = batch
        opt.zero_grad(set_to_none=True)
        seg_l, sr_l, _, _, _ = model(40000, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, segment_sdf=sdf)
        ((1 - beta) * sr_l.mean() + beta * seg_l.mean()).backward()
        opt.step()
    out = {"leg": "step", "hr": a.hr, "batch": a.batch, "steps": a.batches}
    for rep in range(2):                                 # alternate the two feeds, so a drift of the box shows up in both
        ev, wall = timed(lambda: step(fixed), a.batches, a.warmup if rep == 0 else 2)
        out[f"fixed_batch_ms_wall_{rep}"], out[f"fixed_batch_ms_event_{rep}"] = round(wall, 3), round(ev, 3)
        ev, wall = timed(lambda: step(ld.batch(*ld.draw())), a.batches, 2)
        out[f"loader_fed_ms_wall_{rep}"], out[f"loader_fed_ms_event_{rep}"] = round(wall, 3), round(ev, 3)
    f = min(out["fixed_batch_ms_wall_0"], out["fixed_batch_ms_wall_1"])
    l = min(out["loader_fed_ms_wall_0"], out["loader_fed_ms_wall_1"])
    out["loader_share_of_step"] = round((l - f) / l, 4)
    return out


LEGS = {"loader": leg_loader, "kernel": leg_kernel, "step": leg_step}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="one leg in this process (default: all legs, one child process each)")
    ap.add_argument("--hr", type=int, default=224)
    ap.add_argument("--batch", type=int, default=6)
    ap.add_argument("--images", type=int, default=0, help="images in the pool (0: 96 at HR <= 448, else 12)")
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the collected JSON here")
    a = ap.parse_args()
    if a.batches < 50:
        ap.error("--batches must be at least 50")
    if a.leg:
        a.images = a.images or (96 if a.hr <= 448 else 12)
        assert torch.cuda.is_available(), "this benchmark needs an MI355X"
        print(json.dumps(LEGS[a.leg](a)), flush=True)
        return
    results = []
    for leg, hr, batch in (("loader", 224, 6), ("loader", 1792, 8), ("kernel", 224, 6), ("kernel", 1792, 8), ("step", 224, 6)):
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
    doc = json.dumps({"bench": "resident_loader", "legs": results})
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
