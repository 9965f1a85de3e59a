"""Shared by the prediction tests (tests/test_predict_cpu.py, tests/test_predict_gpu.py) and tests/golden/make_predict_golden.py: NumPy
restatements of csbsr_stitch_tiles_u8 and of the border replication of csbsr_gather_crop_u8 as include/csbsr_hip.h states them, the
kernel's case tables, the test images and the host chain of predict_dataset.  No GPU, no reference code."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_tti.npz")
SENTINEL_U8 = np.uint8(0xA5)
SENTINEL_F32 = np.array([0xA5A5A5A5], np.uint32).view(np.float32)[0]        # the same byte, so one fill serves pools and guards


def pool_offsets(dims, C):
    """int64 [n]: first element of image i in a pool of C-channel images = C * (pixels of the images before it)."""
    px = np.asarray(dims, np.int64)[:, 0] * np.asarray(dims, np.int64)[:, 1] * C
    return np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)


def stitch_tiles_numpy(patches, tiles, dims, clip, f32=None, u8=None):
    """patches fp32 [N,C,PH,PW], tiles int [N,8] = (image, dst_y, dst_x, src_y, src_x, th, tw, 0) of a VALID table, dims [n,2] -> the two
    flat pools (fp32 planar per image, uint8 interleaved per image); ``f32`` / ``u8``: what the pools hold before (default: the sentinels),
    so pixels no tile owns keep it."""
    p = np.asarray(patches, np.float32)
    N, C = p.shape[:2]
    dims = np.asarray(dims, np.int64)
    off = pool_offsets(dims, C)
    total = int((dims[:, 0] * dims[:, 1]).sum()) * C
    f32 = np.full(total, SENTINEL_F32, np.float32) if f32 is None else np.array(f32, np.float32).reshape(-1)
    u8 = np.full(total, SENTINEL_U8, np.uint8) if u8 is None else np.array(u8, np.uint8).reshape(-1)
    for n in range(N):
        i, dy, dx, sy, sx, th, tw = (int(v) for v in tiles[n][:7])
        H, W = int(dims[i, 0]), int(dims[i, 1])
        v = p[n, :, sy:sy + th, sx:sx + tw]
        assert v.shape == (C, th, tw) and 0 <= dy and dy + th <= H and 0 <= dx and dx + tw <= W
        f = v.copy()
        if clip:
            f[v > 1] = 1
            f[v < 0] = 0
        c01 = np.where(v > 0, np.where(v < 1, v, np.float32(1)), np.float32(0)).astype(np.float32)        # NaN -> 0
        q = np.trunc(c01 * np.float32(255)).astype(np.uint8)
        f32[off[i]:off[i] + C * H * W].reshape(C, H, W)[:, dy:dy + th, dx:dx + tw] = f
        u8[off[i]:off[i] + C * H * W].reshape(H, W, C)[dy:dy + th, dx:dx + tw] = q.transpose(1, 2, 0)
    return f32, u8


def gather_replicate_numpy(image, y0, x0, h, w):
    """uint8 H x W x C, a window origin that may lie outside the image -> fp32 [C,h,w] = image[clamp(y0 + y), clamp(x0 + x)] / 255."""
    H, W = image.shape[:2]
    ys, xs = np.clip(np.arange(y0, y0 + h), 0, H - 1), np.clip(np.arange(x0, x0 + w), 0, W - 1)
    return np.ascontiguousarray((image[ys][:, xs].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def tile_values(shape, seed, special=False):
    """fp32 ``shape``: uniform on [-0.25, 1.25] with every k / 255 and its two fp32 neighbours planted (as many as fit); ``special`` also
    plants NaN, -0.0, 0, 1, values just outside [0, 1], +-inf and a denormal, several times each."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    v = rng.uniform(-0.25, 1.25, size=n).astype(np.float32)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    planted = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1))])
    if special:
        sp = np.array([np.nan, -0.0, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), -1e-30, 1e-40, np.inf, -np.inf, 7.5, -3.0], np.float32)
        planted = np.concatenate([np.tile(sp, 8), planted])
    pos = rng.permutation(n)[:len(planted)]
    v[pos] = planted[:len(pos)]
    return v.reshape(shape)


# ---------------------------------------------------------------------------------------------------------- kernel cases
# name -> (C, PH, PW, dims of the output images, tile rows); every table is valid (sources inside the patch, destinations inside the image)
def _aligned():
    """(a) two images 24 x 40 and 16 x 24 out of patches 16 x 24: every offset a multiple of 4, whole patches and cut ones, the right-hand
    column of image 0 cut to 16 of 24 columns, its bottom row of tiles to 8 of 16 rows taken from the patch's lower half."""
    rows = [(0, 0, 0, 0, 0, 16, 24, 0), (0, 0, 24, 0, 8, 16, 16, 0), (0, 16, 0, 8, 0, 8, 24, 0), (0, 16, 24, 8, 8, 8, 16, 0),
            (1, 0, 0, 0, 0, 16, 24, 0)]
    return 3, 16, 24, [(24, 40), (16, 24)], rows


def _misaligned(C):
    """(b) patches 10 x 14, source (1, 3), tiles 7 x 9, image widths 13 and 18: no run is aligned anywhere, rows end in tails of 1 pixel."""
    rows = [(0, 0, 0, 1, 3, 7, 9, 0), (0, 7, 4, 1, 3, 7, 9, 0), (1, 1, 0, 1, 3, 7, 9, 0), (1, 2, 9, 1, 3, 7, 9, 0)]
    return C, 10, 14, [(14, 13), (9, 18)], rows


def _unowned():
    """(e) one image 12 x 20 of which only two rectangles are owned; aligned, so whole vector stores sit next to pixels nobody owns."""
    return 3, 8, 12, [(12, 20)], [(0, 0, 4, 0, 0, 8, 12, 0), (0, 8, 0, 4, 4, 4, 8, 0)]


KERNEL_CASES = {"aligned": _aligned(), "misaligned_c3": _misaligned(3), "misaligned_c1": _misaligned(1), "unowned": _unowned(),
                "aligned_c1": (1, 16, 24) + _aligned()[3:]}

# csbsr_gather_crop_u8 windows that leave the image: (image h, w), window (h, w), origins -- negative, past the far edge, both, far outside
GATHER_CASES = [((9, 14), (8, 12), [(-3, -5), (4, 7), (-2, 9), (5, -4), (0, 0), (-20, 30)]),
                ((7, 6), (8, 10), [(-1, -2), (3, 1), (-4, -4), (20, -30)])]


# ---------------------------------------------------------------------------------------------------------- predict_dataset
PREDICT_SIZES = [(16, 24), (21, 17), (5, 9)]         # LR; patch (8, 8): a multiple, a remainder in both axes, smaller than one core


def make_images(sizes, seed):
    """uint8 h x w x 3: a ramp plus noise, so that the stub's SR leaves [0, 1] on both sides and neighbouring pixels differ."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (h, w) in enumerate(sizes):
        ramp = np.linspace(-40, 295, w)[None, :, None] + np.linspace(-30, 30, h)[:, None, None] * (1 + i % 3)
        out.append(np.clip(ramp + rng.uniform(-70, 70, size=(h, w, 3)), 0, 255).astype(np.uint8))
    return out


def host_chain(loader, images, model, to_model, thresholds32):
    """predict_dataset restated on the host from the loader's OWN tables and the decoded ``images``: per unit and per model call the windows (border replication in
    numpy), ``model`` on ``to_model(windows)``, numpy stitching into sentinel-free pools, the saved threshold planes.  Returns per image
    dict(sr_u8, map_u8, map_f32, kernels, planes [S,H,W])."""
    import torch
    out = []
    for unit in loader:
        dims = loader.out_dims
        sub = lambda t: np.concatenate([t[:, :1] - unit.i0, t[:, 1:]], axis=1)          # image column local to the unit
        udims = dims[unit.i0:unit.i1]
        n3, n1 = int((udims[:, 0].astype(np.int64) * udims[:, 1]).sum()) * 3, int((udims[:, 0].astype(np.int64) * udims[:, 1]).sum())
        sr_u8, map_f32, map_u8, kern = np.zeros(n3, np.uint8), np.zeros(n1, np.float32), np.zeros(n1, np.uint8), []
        for a, b in loader.chunks(unit):
            win = np.stack([gather_replicate_numpy(images[g[0]], g[1], g[2], loader.wh, loader.ww) for g in loader.gather[a:b]])
            sr_p, seg_p, kp = model(to_model(win), torch.zeros((b - a, 1, 21, 21)))
            sr_p, seg_p = sr_p.float().cpu().numpy(), seg_p.float().cpu().numpy()
            _, sr_u8 = stitch_tiles_numpy(sr_p, sub(loader.stitch[a:b]), udims, True, u8=sr_u8)
            map_f32, map_u8 = stitch_tiles_numpy(seg_p, sub(loader.stitch[a:b]), udims, False, f32=map_f32, u8=map_u8)
            kern.append(kp.float().cpu().clamp(0, 1))
        kern = torch.cat(kern)
        o1 = pool_offsets(udims, 1)
        for j, i in enumerate(range(unit.i0, unit.i1)):
            H, W = int(udims[j, 0]), int(udims[j, 1])
            m = map_f32[o1[j]:o1[j] + H * W].reshape(H, W)
            d = (m[None] - np.asarray(thresholds32, np.float32)[:, None, None]).astype(np.float32)
            out.append({"name": loader.names[i], "sr_u8": sr_u8[3 * o1[j]:3 * (o1[j] + H * W)].reshape(H, W, 3),
                        "map_u8": map_u8[o1[j]:o1[j] + H * W].reshape(H, W), "map_f32": m,
                        "kernels": kern[int(loader.tile_start[i]) - unit.t0:int(loader.tile_start[i + 1]) - unit.t0],
                        "planes": np.where(d > 0, 255, 0).astype(np.uint8)})
    return out


def load_golden():
    """dict(names, scale, patch, batch_size, lr = decoded uint8 list, batches = [dict(imgs, img_unfold_shape, fnames, joint_ramp)]) as the
    reference's TTICrackDataSetTest under torch's DataLoader delivered them."""
    z = np.load(GOLDEN)
    n, nb = int(z["n"]), int(z["nbatch"])
    return {"names": [str(v) for v in z["names"]], "scale": int(z["scale"]), "patch": tuple(int(v) for v in z["patch"]),
            "batch_size": int(z["batch_size"]), "lr": [z[f"lr_{i}"] for i in range(n)],
            "batches": [{"imgs": z[f"b{j}_imgs"], "img_unfold_shape": z[f"b{j}_img_unfold_shape"], "seg_unfold_shape": z[f"b{j}_seg_unfold_shape"],
                         "fnames": [str(v) for v in z[f"b{j}_fnames"]], "joint_ramp": z[f"b{j}_joint_ramp"]} for j in range(nb)]}


def ramp_patches(n, C, ph, pw):
    """The ramp the fixture pushed through the reference's JointPatch: fp32 arange over [n, C, ph, pw]."""
    return np.arange(n * C * ph * pw, dtype=np.float32).reshape(n, C, ph, pw)
