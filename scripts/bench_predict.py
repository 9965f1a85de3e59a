"""Time the ragged stitch (csrc/eval_io.hip: csbsr_stitch_tiles_u8) and the prediction driver (csbsr_amd/inference.py: predict_dataset) on the GPU.

    python scripts/bench_predict.py                                 # every leg below, each in a child process under its own time limit
    python scripts/bench_predict.py --leg kernel --lr 750 1000 --halo 8

Legs (one JSON line each; the parent prints them again as one JSON object and never opens the GPU itself):
  kernel   csbsr_stitch_tiles_u8 on the SR patches of ONE image (C = 3, clip on, fp32 and uint8 output) next to the torch chain it replaces
           -- per-tile slicing into the output, the two masked clips, mul(255).byte(), permute to HWC -- and next to a device-to-device
           copy_ of the bytes the kernel writes.  The three are timed in turn, ``--rounds`` times over, so the spread of repeated identical
           legs stands beside the differences; bytes are counted from the shapes.
  dataset  predict_dataset without saving next to the route that was there before it: windows cut on the host from the edge-padded decoded
           images (the same tiling, so the outputs can be compared), fp32 / 255 on the host, pageable uploads into the model, torch
           stitching.  Whole passes alternate.
Sizes: LR photographs 750 x 1000 and 448 x 448, scale 4, core 64, halo 0 and 8.  Kernel legs warm up 5 calls and time 50 with events.
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
SCALE, CORE = 4, 64


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


def torch_stitch(patches, rows, out):
    """The chain: every tile's owned rectangle sliced into ``out`` [C,H,W] (rows: host tuples, image column ignored)."""
    for n, (_, dy, dx, sy, sx, th, tw, _) in enumerate(rows):
        out[:, dy:dy + th, dx:dx + tw] = patches[n, :, sy:sy + th, sx:sx + tw]
    return out


def leg_kernel(a):
    from csbsr_amd.data.resident_predict import plan_tiles
    from csbsr_amd.inference import stitch_tiles_u8
    h, w = a.lr
    _, stitch = plan_tiles(h, w, CORE, CORE, a.halo, SCALE)
    rows = [tuple(int(v) for v in r) for r in stitch]
    N, P, H, W = len(rows), SCALE * (CORE + 2 * a.halo), SCALE * h, SCALE * w
    g = torch.Generator(device=DEV).manual_seed(0)
    patches = torch.rand(N, 3, P, P, device=DEV, generator=g) * 1.5 - 0.25
    tiles = torch.from_numpy(stitch).to(DEV)
    off, dims = torch.zeros(1, dtype=torch.int64, device=DEV), torch.tensor([[H, W]], dtype=torch.int32, device=DEV)

    def kernel():
        f32 = torch.empty(3 * H * W, dtype=torch.float32, device=DEV)
        u8 = torch.empty(3 * H * W, dtype=torch.uint8, device=DEV)
        stitch_tiles_u8(patches, tiles, off, dims, clip=True, out_f32=f32, out_u8=u8)
        return f32, u8

    def chain():
        x = torch_stitch(patches, rows, torch.empty(3, H, W, dtype=torch.float32, device=DEV))
        x[x > 1] = 1
        x[x < 0] = 0
        return x, x.mul(255).byte().permute(1, 2, 0).contiguous()
    f32, u8 = kernel()
    cf, cu = chain()
    same = bool(torch.equal(f32.view(3, H, W), cf) and torch.equal(u8.view(H, W, 3), cu))
    df, du = torch.empty_like(f32), torch.empty_like(u8)

    def copy():
        df.copy_(f32)
        du.copy_(u8)
    del cf, cu
    t = {"kernel": [], "chain": [], "copy": []}
    for _ in range(a.rounds):                                # the three in turn, so a drift of the machine shows up in all of them
        for k, fn in (("kernel", kernel), ("chain", chain), ("copy", copy)):
            t[k].append(timed(fn, a.reps, a.warmup))
    spread = {k: max(v) / min(v) - 1 for k, v in t.items()}
    written = f32.numel() * 4 + u8.numel()
    read = 3 * H * W * 4                                     # every owned pixel once (the halo is never read)
    best = {k: min(v) for k, v in t.items()}
    return {"leg": "kernel", "lr": [h, w], "halo": a.halo, "tiles": N, "patch_hr": P, "reps": a.reps, "rounds": a.rounds,
            "stitch_ms": [round(v, 4) for v in t["kernel"]], "torch_chain_ms": [round(v, 4) for v in t["chain"]],
            "copy_ms": [round(v, 4) for v in t["copy"]], "spread": {k: round(v, 4) for k, v in spread.items()},
            "bytes_read": read, "bytes_written": written, "stitch_GBps": round((read + written) / best["kernel"] / 1e6, 1),
            "copy_GBps": round(2 * written / best["copy"] / 1e6, 1), "chain_over_kernel": round(best["chain"] / best["kernel"], 2),
            "kernel_over_copy_time": round(best["kernel"] / best["copy"], 3),
            "kernel_not_slower_than_chain": bool(best["kernel"] <= best["chain"] * (1 + max(spread["kernel"], spread["chain"]))),
            "identical": same}


def leg_dataset(a):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd.inference import predict_dataset
    from csbsr_amd.modeling.build_model import JointModel
    from csbsr_amd.utils.detfill import deterministic_fill
    model = JointModel(base_cfg.clone())
    deterministic_fill(model.state_dict())
    model.eval()
    h, w = a.lr
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(a.images)]
    iset = ResidentImageSet(images, [f"{i:03d}.png" for i in range(a.images)], device=DEV)
    ld = DevicePredictLoader(iset, CORE, SCALE, halo=a.halo, batch_patches=a.batch_patches)
    H, W, halo = SCALE * h, SCALE * w, a.halo

    def resident():
        return [(d["sr_u8"], d["map_u8"], d["map_f32"]) for d in predict_dataset(model, ld)]

    def host():
        """per image: fp32 / 255 and edge padding on the host, the windows of the same tiling cut there, pageable uploads per model call,
        per-tile torch stitching, the two masked clips, mul(255).byte(), permute"""
        out = []
        for i, img in enumerate(images):
            x = np.pad(img.astype(np.float32).transpose(2, 0, 1) / np.float32(255), ((0, 0), (halo, halo + CORE), (halo, halo + CORE)), mode="edge")
            t0, t1 = int(ld.tile_start[i]), int(ld.tile_start[i + 1])
            sr = torch.empty(3, H, W, dtype=torch.float32, device=DEV)
            seg = torch.empty(1, H, W, dtype=torch.float32, device=DEV)
            for c0 in range(t0, t1, a.batch_patches):
                c1 = min(c0 + a.batch_patches, t1)
                win = np.stack([x[:, g[1] + halo:g[1] + halo + ld.wh, g[2] + halo:g[2] + halo + ld.ww] for g in ld.gather[c0:c1]])
                sr_p, seg_p, _ = model(torch.from_numpy(win), torch.zeros((c1 - c0, 1, 21, 21)))
                rows = [tuple(int(v) for v in r) for r in ld.stitch[c0:c1]]
                torch_stitch(sr_p, rows, sr)
                torch_stitch(seg_p, rows, seg)
            sr[sr > 1] = 1
            sr[sr < 0] = 0
            out.append((sr.mul(255).byte().permute(1, 2, 0).contiguous(), seg.clamp(0, 1).mul(255).byte()[0], seg[0]))
        return out

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0
    ra, _ = wall(resident)                                  # warm-up passes: kernel selection, allocator
    rb, _ = wall(host)
    same = all(torch.equal(p, q) for x, y in zip(ra, rb) for p, q in zip(x, y))
    del ra, rb
    t_res, t_host = [], []
    for _ in range(a.passes):                               # alternate, so a drift of the machine shows up in both
        t_res.append(wall(resident)[1])
        t_host.append(wall(host)[1])
    ips = lambda ts_: [round(a.images / t, 3) for t in ts_]
    return {"leg": "dataset", "images": a.images, "lr": [h, w], "halo": halo, "batch_patches": a.batch_patches, "tiles_per_image": int(ld.tile_start[1]),
            "passes": a.passes, "resident_images_per_s": ips(t_res), "host_fed_images_per_s": ips(t_host),
            "resident_images_per_s_best": round(a.images / min(t_res), 3), "host_fed_images_per_s_best": round(a.images / min(t_host), 3),
            "speedup_best": round(min(t_host) / min(t_res), 3), "resident_spread": round(max(t_res) / min(t_res) - 1, 4),
            "host_fed_spread": round(max(t_host) / min(t_host) - 1, 4), "outputs_identical": bool(same)}


LEGS = {"kernel": leg_kernel, "dataset": leg_dataset}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="one leg in this process (default: all legs, one child process each)")
    ap.add_argument("--lr", type=int, nargs=2, default=[750, 1000], help="LR image height and width")
    ap.add_argument("--halo", type=int, default=0)
    ap.add_argument("--images", type=int, default=4, help="dataset leg: images in the set")
    ap.add_argument("--batch-patches", type=int, default=16, help="dataset leg: windows per model call")
    ap.add_argument("--passes", type=int, default=3, help="dataset leg: timed passes over the set per feed")
    ap.add_argument("--rounds", type=int, default=5, help="kernel leg: times every timing is repeated")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the collected JSON here")
    a = ap.parse_args()
    if a.reps < 50:
        ap.error("--reps must be at least 50")
    if a.leg:
        assert torch.cuda.is_available(), "this benchmark needs an MI355X"
        print(json.dumps(LEGS[a.leg](a)), flush=True)
        return
    plan = [("kernel", lr, halo, 0) for lr in ((750, 1000), (448, 448)) for halo in (0, 8)]
    plan += [("dataset", (750, 1000), 0, 2), ("dataset", (750, 1000), 8, 2), ("dataset", (448, 448), 0, 8), ("dataset", (448, 448), 8, 8)]
    results = []
    for leg, lr, halo, images in plan:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--lr", str(lr[0]), str(lr[1]), "--halo", str(halo), "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--images", str(images or a.images), "--passes", str(a.passes),
               "--batch-patches", str(a.batch_patches)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
        except subprocess.TimeoutExpired:
            print(f"leg {leg} lr {lr} halo {halo}: no result within {LEG_TIMEOUT_S} s; stopping", file=sys.stderr)
            sys.exit(124)
        if r.returncode != 0:                            # nothing more is started on the GPU after a failed leg
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            print(f"leg {leg} lr {lr} halo {halo} failed with status {r.returncode}; stopping", file=sys.stderr)
            sys.exit(r.returncode if r.returncode > 0 else 1)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    doc = json.dumps({"bench": "predict", "legs": results})
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
