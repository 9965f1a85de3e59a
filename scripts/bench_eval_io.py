"""Time the evaluation outputs (csrc/eval_io.hip) and the whole-test-set evaluation (csbsr_amd/inference.py: evaluate_dataset) on the GPU.

    python scripts/bench_eval_io.py                                 # every leg below, each in a child process under its own time limit
    python scripts/bench_eval_io.py --leg kernel --hr 1792 --batch 8

Legs (one JSON line each; the parent prints them again as one JSON object and never opens the GPU itself):
  kernel   csbsr_stitch_clip_u8 (fp32 and uint8 output, clip on) and csbsr_threshold_planes_u8 (the 11 saved thresholds), each next to the
           torch chain it replaces -- JointPatch + two masked assignments + mul(255).byte() + permute to HWC; (pred - th > 0) for the 11
           thresholds + .byte() * 255 -- and next to a device-to-device copy_ of the bytes the kernel writes.  Sizes: B = 12 of 448^2 as one
           patch (test.py's default) and B = 8 of 1792^2 as 16 patches of 448^2.
  dataset  evaluate_dataset without saving over a 48-image synthetic 448^2 test set, config-2 model, batch 12, next to the same loop fed
           the way it had to be fed before: host fp32 tensors per batch into evaluate_batch.  Whole passes alternate between the two;
           images per second of every pass are printed, so the run-to-run spread is visible beside the difference.
Kernel legs warm up first and time with events over >= 50 calls.
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
SAVE_IDX = [0, 9, 19, 29, 39, 49, 59, 69, 79, 89, 98]


def timed(fn, n, warmup):
    """fn() n times after `warmup` calls: event ms per call between two synchronisations."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def leg_kernel(a):
    from csbsr_amd.data.patch_sampler import JointPatch
    from csbsr_amd.inference import THRESHOLDS, stitch_clip_u8, threshold_planes_u8
    B, H, p = a.batch, a.hr, 448
    n = H // p
    g = torch.Generator(device=DEV).manual_seed(0)
    patches = torch.rand(B * n * n, 3, p, p, device=DEV, generator=g) * 1.5 - 0.25
    shape = np.array([B, 1, n, n, 3, p, p])
    joint = JointPatch()

    def chain():
        x = joint(patches, shape)
        x[x > 1] = 1
        x[x < 0] = 0
        return x, x.mul(255).byte().permute(0, 2, 3, 1).contiguous()
    f32, u8 = stitch_clip_u8(patches, shape, clip=True, want_u8=True)
    cf, cu = chain()
    same_stitch = bool(torch.equal(f32, cf) and torch.equal(u8, cu))
    t_k = timed(lambda: stitch_clip_u8(patches, shape, clip=True, want_u8=True), a.reps, a.warmup)
    t_c = timed(chain, a.reps, a.warmup)
    df, du = torch.empty_like(f32), torch.empty_like(u8)

    def copy():
        df.copy_(f32)
        du.copy_(u8)
    t_d = timed(copy, a.reps, a.warmup)
    out = {"leg": "kernel", "hr": H, "batch": B, "patches_per_image": n * n, "reps": a.reps,
           "stitch_ms": round(t_k, 4), "stitch_torch_chain_ms": round(t_c, 4), "stitch_copy_ms": round(t_d, 4),
           "stitch_bytes_written": f32.numel() * 4 + u8.numel(), "stitch_chain_over_kernel": round(t_c / t_k, 2),
           "stitch_over_copy_time": round(t_k / t_d, 3), "stitch_identical": same_stitch}
    del cf, cu, df, du, f32, u8, patches
    pred = torch.rand(B, H, H, device=DEV, generator=g)
    th = torch.tensor([float(t) for t in THRESHOLDS], dtype=torch.float32)[SAVE_IDX].to(DEV)
    th_map, zero = th.view(1, -1, 1, 1), torch.zeros(1, device=DEV)

    def chain_planes():
        return (pred[:, None] - th_map > zero).byte() * 255
    planes = threshold_planes_u8(pred, th)
    same_planes = bool(torch.equal(planes, chain_planes()))
    t_k = timed(lambda: threshold_planes_u8(pred, th), a.reps, a.warmup)
    t_c = timed(chain_planes, a.reps, a.warmup)
    dp = torch.empty_like(planes)
    t_d = timed(lambda: dp.copy_(planes), a.reps, a.warmup)
    out.update({"planes_ms": round(t_k, 4), "planes_torch_chain_ms": round(t_c, 4), "planes_copy_ms": round(t_d, 4),
                "planes_bytes_written": planes.numel(), "planes_chain_over_kernel": round(t_c / t_k, 2),
                "planes_over_copy_time": round(t_k / t_d, 3), "planes_identical": same_planes})
    return out


def make_testset(n, hr, scale, seed=0):
    rng = np.random.default_rng(seed)
    lr = hr // scale
    images = [rng.integers(0, 256, size=(hr, hr, 3), dtype=np.uint8) for _ in range(n)]
    lrs = [rng.integers(0, 256, size=(lr, lr, 3), dtype=np.uint8) for _ in range(n)]
    masks = []
    for _ in range(n):
        m = np.zeros((hr, hr), np.uint8)
        m[hr // 2 - 3:hr // 2 + 3, :] = 255
        x = int(rng.integers(0, hr - 5))
        m[:, x:x + 5] = 255
        masks.append(m)
    r = np.arange(21) - 10
    kernels = []
    for i in range(n):
        gk = np.exp(-0.5 * ((r[None, :] / (1.0 + 0.05 * i)) ** 2 + (r[:, None] / (3.0 - 0.03 * i)) ** 2))
        kernels.append(np.round(gk / gk.max() * 255).astype(np.uint8))
    return images, masks, lrs, kernels, [f"{i:03d}.jpg" for i in range(n)]


def leg_dataset(a):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.patch_sampler import SplitPatch
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet, kernel_target
    from csbsr_amd.inference import evaluate_batch, evaluate_dataset
    from csbsr_amd.modeling.build_model import JointModel
    from csbsr_amd.utils.detfill import deterministic_fill
    cfg = base_cfg.clone()
    model = JointModel(cfg)
    deterministic_fill(model.state_dict())
    model.eval()
    hr, scale, B, n = 448, 4, a.batch, a.images
    images, masks, lrs, kernels, names = make_testset(n, hr, scale)
    ts = ResidentTestSet(images, masks, lrs, kernels, names, device=DEV)

    def resident():
        return evaluate_dataset(model, DeviceTestLoader(ts, hr, scale, B))

    def host():
        """the loop the code before evaluate_dataset allowed: CrackDataSetTest's host work per image (the files already decoded),
        collated host tensors into evaluate_batch, numpy appends"""
        sp = SplitPatch(B, 3, hr // scale, hr // scale)
        acc = {k: [] for k in ("psnr", "ssim", "kernel_psnr", "iou")}
        for i0 in range(0, n, B):
            idx = range(i0, min(i0 + B, n))
            sr_t = torch.stack([torch.from_numpy(images[i].astype(np.float32)).permute(2, 0, 1) / 255 for i in idx])
            m = torch.stack([torch.from_numpy(masks[i][:, :, None].astype(np.float32)).permute(2, 0, 1) / 255 for i in idx])
            pats, shapes = zip(*(sp(torch.from_numpy(lrs[i].astype(np.float32)).permute(2, 0, 1) / 255) for i in idx))
            img_shape = shapes[0].copy()
            img_shape[[5, 6]] *= scale
            seg_shape = img_shape.copy()
            seg_shape[[1, 4]] = 1
            kt = torch.stack([kernel_target(kernels[i]).expand(pats[0].shape[0], 21, 21) for i in idx])
            r = evaluate_batch(model, torch.stack(pats), img_shape, seg_shape, sr_t, m, kt, ksize=21)
            for k in acc:
                acc[k].append(r[k])
        return {k: np.concatenate(v) for k, v in acc.items()}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    ra, _ = wall(resident)                                  # warm-up passes: kernel selection, allocator, pinned buffers
    rb, _ = wall(host)
    same = all(ra[k].tobytes() == rb[k].tobytes() for k in ("psnr", "ssim", "kernel_psnr", "iou"))
    t_res, t_host = [], []
    for _ in range(a.passes):                               # alternate, so a drift of the machine shows up in both
        t_res.append(wall(resident)[1])
        t_host.append(wall(host)[1])
    ips = lambda ts_: [round(n / t, 2) for t in ts_]
    return {"leg": "dataset", "images": n, "hr": hr, "batch": B, "passes": a.passes, "resident_images_per_s": ips(t_res),
            "host_fed_images_per_s": ips(t_host), "resident_images_per_s_best": round(n / min(t_res), 2),
            "host_fed_images_per_s_best": round(n / min(t_host), 2), "speedup_best": round(min(t_host) / min(t_res), 3),
            "resident_spread": round(max(t_res) / min(t_res) - 1, 4), "host_fed_spread": round(max(t_host) / min(t_host) - 1, 4),
            "outputs_identical": bool(same), "summary": ra["summary"]}


LEGS = {"kernel": leg_kernel, "dataset": leg_dataset}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="one leg in this process (default: all legs, one child process each)")
    ap.add_argument("--hr", type=int, default=448, help="kernel leg: image side, a multiple of 448")
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--images", type=int, default=48, help="dataset leg: images in the test set")
    ap.add_argument("--passes", type=int, default=5, help="dataset leg: timed passes over the test set per feed")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the collected JSON here")
    a = ap.parse_args()
    if a.reps < 50:
        ap.error("--reps must be at least 50")
    if a.hr % 448:
        ap.error("--hr must be a multiple of 448")
    if a.leg:
        assert torch.cuda.is_available(), "this benchmark needs an MI355X"
        print(json.dumps(LEGS[a.leg](a)), flush=True)
        return
    results = []
    for leg, hr, batch in (("kernel", 448, 12), ("kernel", 1792, 8), ("dataset", 448, 12)):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--hr", str(hr), "--batch", str(batch), "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--images", str(a.images), "--passes", str(a.passes)]
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
    doc = json.dumps({"bench": "eval_io", "legs": results})
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
