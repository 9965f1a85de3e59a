"""Shared by the evaluation-output tests and tests/golden/make_eval_golden.py: NumPy restatements of csbsr_stitch_clip_u8,
csbsr_threshold_planes_u8, of what CrackDataSetTest + TestTransforms + SplitPatch deliver per image and of get_retinal_seg_metrics; the
CPU torch chains the two kernels replace; the kernels' test cases; and the deterministic stub model of the evaluate_dataset tests.
No GPU, no reference code."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_testset.npz")
THRESHOLDS = [i * 0.01 for i in range(1, 100)]
SAVE_IDX = [0, 9, 19, 29, 39, 49, 59, 69, 79, 89, 98]

# (B, C, nH, nW, ph, pw): aligned rows; the identity; pw % 4 != 0 with odd bases; patches narrower than a 16-run; long rows
STITCH_SHAPES = [(2, 3, 2, 3, 8, 12), (3, 3, 1, 1, 16, 24), (2, 1, 3, 2, 5, 7), (1, 3, 2, 2, 4, 6), (2, 1, 1, 4, 64, 16)]
PLANE_HW = [17 * 23, 64 * 64]


# ------------------------------------------------------------------------------------------------------------ the two kernels
def stitch_numpy(patches, B, C, nH, nW, ph, pw, clip):
    """patches fp32 [B*nH*nW, C, ph, pw] -> (fp32 [B,C,H,W], uint8 [B,H,W,C]) as include/csbsr_hip.h states them."""
    v = np.asarray(patches, np.float32).reshape(B, nH, nW, C, ph, pw).transpose(0, 3, 1, 4, 2, 5).reshape(B, C, nH * ph, nW * pw)
    f32 = v.copy()
    if clip:
        f32[v > 1] = 1
        f32[v < 0] = 0
    c = np.where(v > 0, np.where(v < 1, v, np.float32(1)), np.float32(0)).astype(np.float32)        # NaN -> 0
    u8 = np.trunc(c * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1)
    return f32, np.ascontiguousarray(u8)


def stitch_torch(patches, B, C, nH, nW, ph, pw, clip):
    """The chain the kernel replaces, in CPU torch: JointPatch's view / permute / contiguous (patch_sampler.py:30-51), the two masked
    assignments (inference.py:94-95), ToPILImage's mul(255).byte() on the CLIPPED image and its CHW -> HWC."""
    p = torch.as_tensor(patches).view(-1, 1, nH, nW, C, ph, pw)
    x = p.permute(0, 1, 4, 2, 5, 3, 6).contiguous().view(-1, C, nH * ph, nW * pw)
    c = x.clone()
    c[c > 1] = 1
    c[c < 0] = 0
    u8 = c.mul(255).byte().permute(0, 2, 3, 1).contiguous()
    return (c if clip else x), u8


def stitch_values(shape, seed):
    """fp32 [B*nH*nW, C, ph, pw]: uniform on [-0.25, 1.25] with planted 0, 1, -0.0, 1e-40 and every k / 255 with its two fp32 neighbours
    (as many as fit, at seeded positions)."""
    B, C, nH, nW, ph, pw = shape
    rng = np.random.default_rng(seed)
    n = B * nH * nW * C * ph * pw
    v = rng.uniform(-0.25, 1.25, size=n).astype(np.float32)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    planted = np.concatenate([np.array([0.0, 1.0, -0.0, 1e-40], np.float32), k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1))])
    pos = rng.permutation(n)[:len(planted)]
    v[pos] = planted[:len(pos)]
    return v.reshape(B * nH * nW, C, ph, pw)


def thresholds32(thresholds=THRESHOLDS):
    return torch.tensor([float(t) for t in thresholds], dtype=torch.float32).numpy()          # == torch.Tensor(thresholds)


def plane_thresholds(S):
    """S = 1: one threshold; 11: the saved ones as torch.Tensor(thresholds) rounds them; 16: sixteen in DEscending order."""
    th = thresholds32()
    return {1: th[49:50], 11: th[SAVE_IDX], 16: th[[97, 90, 83, 77, 70, 64, 58, 51, 45, 38, 31, 25, 18, 12, 5, 0]]}[S].copy()


def planes_numpy(pred, th):
    """pred fp32 [N, hw], th fp32 [S] -> uint8 [N, S, hw]: 255 where the fp32 difference is > 0."""
    d = (np.asarray(pred, np.float32)[:, None, :] - np.asarray(th, np.float32)[None, :, None]).astype(np.float32)
    return np.where(d > 0, 255, 0).astype(np.uint8)


def planes_torch(pred, th):
    """inference.py:111 on the CPU, then ToPILImage of the 0 / 1 plane."""
    p, t = torch.as_tensor(pred), torch.as_tensor(th)
    bi = (p[:, None, :] - t.view(1, -1, 1) > torch.Tensor([0])).float()
    return bi.mul(255).byte()


def plane_values(N, hw, th, seed):
    """uniform [0, 1) with every threshold, its two fp32 neighbours, 0, 1 and NaN planted in every map."""
    rng = np.random.default_rng(seed)
    v = rng.random((N, hw)).astype(np.float32)
    planted = np.concatenate([th, np.nextafter(th, np.float32(2)), np.nextafter(th, np.float32(-1)), np.array([0, 1, np.nan], np.float32)])
    for n in range(N):
        v[n, rng.permutation(hw)[:len(planted)]] = planted
    return v


# ------------------------------------------------------------------------------------------------------------ the test set
def anisotropic_kernels(n, K=21, first=0):
    """uint8 K x K images of n distinct anisotropic Gaussians scaled to max 255."""
    out = []
    r = np.arange(K) - K // 2
    yy, xx = np.meshgrid(r, r, indexing="ij")
    for i in range(first, first + n):
        sx, sy, th = 1.0 + 0.45 * i, 3.6 - 0.3 * i, 0.37 * i + 0.2
        u, v = np.cos(th) * xx + np.sin(th) * yy, -np.sin(th) * xx + np.cos(th) * yy
        g = np.exp(-0.5 * ((u / sx) ** 2 + (v / sy) ** 2))
        out.append(np.round(g / g.max() * 255).astype(np.uint8))
    return out


def make_testset(seed, n, H, W, scale, zero_mask=None):
    """(hr, masks, lr, kernels, names): smooth-plus-noise LR images whose channel mean sweeps [0, 1], noise HR images holding every byte,
    masks of a band and a blob with a soft edge (bytes other than 0 / 255); ``zero_mask``: index of an all-zero mask."""
    rng = np.random.default_rng(seed)
    hr = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(n)]
    h, w = H // scale, W // scale
    lr, masks = [], []
    for i in range(n):
        ramp = np.linspace(-40, 295, w)[None, :, None] + np.linspace(-30, 30, h)[:, None, None] * (1 + i % 3)
        lr.append(np.clip(ramp + rng.uniform(-70, 70, size=(h, w, 3)), 0, 255).astype(np.uint8))
        m = np.zeros((H, W), np.uint8)
        m[H // 2 - 3:H // 2 + 3, :] = 255
        m[H // 2 - 4, :], m[H // 2 + 3, :] = 130, 254
        x0 = int(rng.integers(W // 2, W - 14))
        m[4:16, x0:x0 + 12] = 255
        if zero_mask == i:
            m[:] = 0
        masks.append(m)
    return hr, masks, lr, anisotropic_kernels(n), [f"img_{i:02d}.jpg" for i in range(n)]


def reference_item_numpy(hr, mask, lr, kernel, image_size, scale, batch_size, num_classes=1):
    """What CrackDataSetTest.__getitem__ returns for one image (crack_dataset.py:86-139 with TestTransforms), restated:
    (img [nPatch,3,ph,pw], sr_target [3,H,W], seg_target [1,H,W], blur_kernel [nPatch,K,K], img_unfold_shape, seg_unfold_shape)."""
    f255 = np.float32(255)
    sr = hr.astype(np.float32).transpose(2, 0, 1) / f255
    seg = mask[None].astype(np.float32) / f255
    k = kernel[None].astype(np.float32) / f255
    k = k / torch.sum(torch.from_numpy(k)).numpy()              # (the reference's own reduction: torch.sum in fp32)
    x = lr.astype(np.float32).transpose(2, 0, 1) / f255
    ph, pw = int(image_size[0] / scale), int(image_size[1] / scale)
    nH, nW = x.shape[1] // ph, x.shape[2] // pw
    p = x[:, :nH * ph, :nW * pw].reshape(3, nH, ph, nW, pw).transpose(1, 3, 0, 2, 4).reshape(nH * nW, 3, ph, pw)
    img_shape = np.array([batch_size, 1, nH, nW, 3, ph * scale, pw * scale], dtype=np.int64)
    seg_shape = img_shape.copy()
    seg_shape[[1, 4]] = num_classes
    return np.ascontiguousarray(p), sr, seg, np.ascontiguousarray(np.broadcast_to(k, (nH * nW,) + k.shape[1:])), img_shape, seg_shape


def load_golden():
    """{"A": set, "B": set}; a set = dict(names, hr, mask, lr, kernel (decoded uint8 lists), image_size, scale, batch_size,
    batches = [dict(imgs, sr_targets, masks, kernel_targets, fnames, img_unfold_shape, seg_unfold_shape)] as the reference's DataLoader
    collated them)."""
    z = np.load(GOLDEN)
    out = {}
    for s in ("A", "B"):
        n, nb = int(z[f"{s}_n"]), int(z[f"{s}_nbatch"])
        out[s] = {"names": [str(v) for v in z[f"{s}_names"]], "image_size": tuple(int(v) for v in z[f"{s}_image_size"]),
                  "scale": int(z[f"{s}_scale"]), "batch_size": int(z[f"{s}_batch_size"]),
                  **{k: [z[f"{s}_{k}_{i}"] for i in range(n)] for k in ("hr", "mask", "lr", "kernel")},
                  "batches": [{**{k: z[f"{s}_b{j}_{k}"] for k in ("imgs", "sr_targets", "masks", "kernel_targets", "img_unfold_shape",
                                                                   "seg_unfold_shape")},
                               "fnames": [str(v) for v in z[f"{s}_b{j}_fnames"]]} for j in range(nb)]}
    return out


# ------------------------------------------------------------------------------------------------------------ the stub model
_RAMP = {}


def stub_model(imgs, dummy=None, sr_targets=None):
    """A deterministic stand-in for JointModel.eval() made of exactly rounded elementwise fp32 operations, so the CPU and the device give
    the same bits: SR = nearest x4 of the LR patch plus a fixed ramp (leaves [0, 1] on both sides), the map = ((r + g) + b) * fp32(1/3) of
    the SR patch, the kernels = fixed Gaussians by position in the batch."""
    n, _, h, w = imgs.shape
    key = (h, w)
    if key not in _RAMP:
        y, x, c = torch.arange(4 * h).view(1, -1, 1), torch.arange(4 * w).view(1, 1, -1), torch.arange(3).view(-1, 1, 1)
        _RAMP[key] = (((y * 7 + x * 3 + c * 5) % 32 - 12).to(torch.float32) / 64)
    sr = imgs.repeat_interleave(4, dim=2).repeat_interleave(4, dim=3) + _RAMP[key].to(imgs.device)
    seg = ((sr[:, 0:1] + sr[:, 1:2]) + sr[:, 2:3]) * torch.tensor(1 / 3, dtype=torch.float32, device=imgs.device)
    k = np.stack(anisotropic_kernels(n, first=1)).astype(np.float32)
    k = torch.from_numpy(k / k.sum(axis=(1, 2), keepdims=True) * np.float32(1.5)).view(n, 1, 21, 21)       # (peaks above and below 1 / 255)
    return sr, seg, k.to(imgs.device)


def retinal_numpy(seg_bin, masks):
    """get_retinal_seg_metrics (retinal_metrics.py) restated per image: seg_bin [B,H,W] of 0 / 1, masks fp32 [B,1,H,W] = byte / 255."""
    seg = np.asarray(seg_bin).astype(np.int16)
    ground = np.asarray(masks)[:, 0].astype(np.int16)
    tp = np.sum(ground * seg, axis=(1, 2))
    tn = np.sum((ground == 0).astype(np.int16) * (seg == 0).astype(np.int16), axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = (tp + tn) / (ground.size / ground.shape[0])
        sens = tp / np.sum(ground, axis=(1, 2))
        spec = tn / np.sum((ground == 0).astype(np.int16), axis=(1, 2))
    np.place(sens, sens == np.inf, 1)
    np.place(spec, spec == np.inf, 1)
    return acc, sens, spec


def cpu_chain(items, batch):
    """One batch of the evaluation loop on the CPU with the stub: items = reference_item_numpy tuples of the batch's images ->
    dict(sr_u8 [B,H,W,3], raw_u8 [B,H,W], planes [B,11,H,W] uint8, seg [B,1,H,W], sr [B,3,H,W] clipped, kernel_preds clipped)."""
    imgs = torch.from_numpy(np.concatenate([it[0] for it in items]))
    sr_p, seg_p, kp = stub_model(imgs)
    s, g = [int(v) for v in items[0][4]], [int(v) for v in items[0][5]]
    sr, sr_u8 = stitch_torch(sr_p, batch, 3, s[2], s[3], s[5], s[6], True)
    seg, _ = stitch_torch(seg_p, batch, 1, g[2], g[3], g[5], g[6], False)
    raw_u8 = seg.clamp(0, 1).mul(255).byte()[:, 0]
    th = torch.from_numpy(thresholds32()[SAVE_IDX])
    planes = planes_torch(seg.view(batch, -1), th).view(batch, len(SAVE_IDX), *seg.shape[2:])
    kp = kp.clone()
    kp[kp > 1] = 1
    kp[kp < 0] = 0
    return {"sr_u8": sr_u8.numpy(), "raw_u8": raw_u8.numpy(), "planes": planes.numpy(), "seg": seg, "sr": sr, "kernel_preds": kp}
