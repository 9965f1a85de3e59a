"""Shared by tests/test_metric_cases_cpu.py, tests/test_metrics_exact_gpu.py and tests/test_aux_rows_gpu.py: fp64 restatements of the
evaluation metrics and of the blur-kernel synthesis (csrc/data_ops.hip), and input builders for the chunked loss reductions
(csbsr_l1_fwd_bwd, csbsr_plane_reduce, csbsr_segloss_reduce / _finish).  No GPU.  Everything here is written from the formulas:

  IoU     inter = #{(pred - t > 0) & (mask > 0.5)}, union = #{(pred - t > 0) | (mask > 0.5)}, the subtraction in fp32 on the fp32-rounded
          thresholds (``torch.Tensor(thresholds)`` rounds them before the broadcast subtraction); iou = (inter + 1e-5) / (union + 1e-5).
  PSNR    10 log10(1 / mean_{C,H,W} (a - b)^2).
  SSIM    11-tap sigma-1.5 window (built in fp32, outer product in fp32, then widened), depthwise, zero padding 5, C1 = 0.01^2,
          C2 = 0.03^2, mean over (C, H, W).
  blur    exp(-(a x^2 + 2 b x y + c y^2)) / sum on linspace(-r, r, K), r = int(K / 2), with the rotated inverse-variance form a, b, c.

The lattice builders return inputs whose sums are exactly representable: every term is an integer multiple of one power of two and
the sum of the magnitudes stays below 2^24 such units, so an fp32 summation in ANY order is exact and a kernel can be asked for
bit-equality.  Each builder asserts that bound on the host before a test relies on it.

Known limit: csbsr_iou_sweep returns ``inter`` / ``union`` as fp32, so they are exact only up to 2^24 pixels per sample (a 4096^2
image); ``iou`` itself is formed from the integer counts in fp64 and does not share the limit.  Not tested: it needs a 4097^2 image.
"""
import math
import os
import re

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csbsr_amd", "csrc")
FP32_EXACT = 1 << 24          # integers below this are exact in fp32


# ------------------------------------------------------------------------------------------- IoU sweep

def thresholds32(thresholds):
    """the fp32 roundings ``torch.Tensor(thresholds)`` holds"""
    return np.asarray([float(t) for t in thresholds], np.float32)


def many_thresholds(T):
    """T strictly ascending fp32 thresholds inside (0, 1), far enough apart that the fp32 neighbours of one are not another"""
    th = np.linspace(0.001, 0.999, T).astype(np.float32) if T > 1 else np.asarray([0.5], np.float32)
    assert np.all(th[1:] > np.nextafter(th[:-1], np.float32(np.inf)))
    return th


def ref_iou_counts(pred, mask, th32):
    """integer (inter, union) [B, T] of fp32 ``pred`` / ``mask`` [B, hw]"""
    pred, mask, th32 = np.asarray(pred), np.asarray(mask), np.asarray(th32)
    assert pred.dtype == np.float32 and mask.dtype == np.float32 and th32.dtype == np.float32
    pred, mask = pred.reshape(pred.shape[0], -1), mask.reshape(mask.shape[0], -1)
    fg = mask > np.float32(0.5)
    inter = np.zeros((pred.shape[0], len(th32)), np.int64)
    union = np.zeros_like(inter)
    with np.errstate(invalid="ignore"):
        for j, t in enumerate(th32):
            o = (pred - t) > 0                     # fp32 - fp32: NaN compares false, +inf exceeds every threshold
            inter[:, j] = (o & fg).sum(1)
            union[:, j] = (o | fg).sum(1)
    return inter, union


def ref_iou(inter, union, smooth=1e-5):
    return (np.asarray(inter, np.float64) + smooth) / (np.asarray(union, np.float64) + smooth)


def ulp32(x):
    """spacing of fp32 at |x| (fp64 array)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


MASK_VALUES = np.asarray([0.0, 1.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.49], np.float32)      # fg: 1 and 0.5 + 1 ulp


def tie_pool(th32):
    """the prediction values that sit on a decision: every threshold, its two fp32 neighbours, the ends of the range, values outside
    it and the non-finite ones"""
    th32 = np.asarray(th32, np.float32)
    up, dn = np.nextafter(th32, np.float32(np.inf)), np.nextafter(th32, np.float32(-np.inf))
    return np.concatenate([th32, up, dn, np.asarray([0.0, 1.0, -0.25, 1.5, np.inf, -np.inf, np.nan], np.float32)])


def iou_tie_inputs(B, hw, th32, seed=0, background_sample=None):
    """(pred, mask) fp32 [B, hw].  Every third pixel holds a value of tie_pool paired with one of MASK_VALUES: special j of sample n is
    (pool[(j + 7 n) % P], MASK_VALUES[((j + 7 n) // P) % 5]), so each pool value meets each mask value once per 5 P specials, wherever
    the chunk boundaries fall; the other pixels are uniform noise in [-0.1, 1.1) with a random mask value.  ``background_sample``: that
    sample becomes all background (mask 0 / 0.5 / 0.49) with every prediction at or below the lowest threshold."""
    rng = np.random.default_rng(seed)
    pool = tie_pool(th32)
    P = len(pool)
    pred = (rng.random((B, hw), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)).astype(np.float32)
    mask = MASK_VALUES[rng.integers(0, 5, size=(B, hw))]
    pos = np.arange(0, hw, 3)
    for n in range(B):
        j = np.arange(len(pos)) + 7 * n
        pred[n, pos] = pool[j % P]
        mask[n, pos] = MASK_VALUES[(j // P) % 5]
    if background_sample is not None:
        t0 = np.float32(th32[0])
        low = np.asarray([t0, np.nextafter(t0, np.float32(-np.inf)), 0.0, -0.25, -np.inf, np.nan, t0 / 2], np.float32)
        pred[background_sample] = low[rng.integers(0, len(low), size=hw)]
        mask[background_sample] = np.asarray([0.0, 0.5, 0.49], np.float32)[rng.integers(0, 3, size=hw)]
    return pred, mask


def tie_coverage_gaps(pred, mask, th32):
    """for ONE sample: the (threshold index, which) pairs -- which in 'at', 'above', 'below' -- that do not occur both in foreground
    and in background"""
    th32 = np.asarray(th32, np.float32)
    fg = mask > np.float32(0.5)
    gaps = []
    vals = {"at": th32, "above": np.nextafter(th32, np.float32(np.inf)), "below": np.nextafter(th32, np.float32(-np.inf))}
    pf, pb = set(pred[fg].tolist()), set(pred[~fg].tolist())
    for which, v in vals.items():
        for i, x in enumerate(v.tolist()):
            if x not in pf or x not in pb:
                gaps.append((i, which))
    return gaps


# (B, hw): a single pixel; either side of one pass of 256 threads; the last single-chunk size; two chunks with a ragged last one
# (per = 32769: the `end` clamp); three even chunks (131841 = 3 * 43947); three chunks with a ragged last one (per = 43948); more
# samples than the fixture, two ragged chunks (per = 33033)
IOU_SHAPES = [(1, 1), (3, 255), (3, 257), (2, 65536), (2, 65537), (2, 257 * 513), (2, 257 * 513 + 1), (5, 66065)]
IOU_EXTRA_T = [(2, 65537, 1), (2, 65537, 2), (2, 66065, 1024)]          # (B, hw, T) beside T = 99 everywhere


# ------------------------------------------------------------------------------------------- PSNR / SSIM

def _ssim_window(channels):
    """[channels, 1, 11, 11] fp32: the normalised 11-tap Gaussian of sigma 1.5 (2 sigma^2 = 4.5), rounded to fp32 before it is normalised,
    and its fp32 outer product -- one copy per channel for a depthwise convolution"""
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], dtype=torch.float32)
    g = g / g.sum()
    return torch.outer(g, g).repeat(channels, 1, 1, 1)


def ref_psnr_ssim(a, b, dtype=torch.float64):
    """(psnr [N], ssim [N]) numpy fp64 of two [N, C, H, W] batches; ``dtype=torch.float32`` evaluates the same formulas in fp32 (the
    yardstick for how far any fp32 evaluation sits from fp64)"""
    a, b = torch.as_tensor(np.asarray(a)).to(dtype), torch.as_tensor(np.asarray(b)).to(dtype)
    C = a.shape[1]
    mse = ((a - b) ** 2).mean((1, 2, 3))
    with np.errstate(divide="ignore"):
        psnr = 10 * np.log10(1 / mse.double().numpy())
    w = _ssim_window(C).to(dtype)
    conv = lambda x: F.conv2d(x, w, padding=5, groups=C)
    mu1, mu2 = conv(a), conv(b)
    mu1s, mu2s, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = conv(a * a) - mu1s, conv(b * b) - mu2s, conv(a * b) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1s + mu2s + C1) * (s1 + s2 + C2))
    return psnr, m.mean((1, 2, 3)).double().numpy()


# (N, C, H, W): a single pixel; smaller than the 11-tap window; the kernel-PSNR call of evaluate_batch; exactly one 32 x 8 tile; one
# pixel over in both directions; the fixture's size; 3 * 12 * 29 = 1044 partial rows per sample -- above the 1024 of one fold chunk
IMG_SHAPES = [(2, 1, 1, 1), (2, 3, 5, 5), (4, 1, 21, 21), (2, 3, 8, 32), (2, 3, 9, 33), (1, 2, 40, 52), (2, 3, 93, 925)]


def fold_rows_per_chunk():
    """rows one first-level block of csbsr_sum_partials_batched folds (RPC, csrc/elementwise.hip): more rows take the two-level path"""
    with open(os.path.join(CSRC, "elementwise.hip")) as f:
        m = re.search(r"const int RPC = (\d+);", f.read())
    assert m, "RPC not found in csrc/elementwise.hip"
    return int(m.group(1))


def partial_rows(C, H, W):
    """partial rows per sample csbsr_psnr_ssim hands to the fold (one per 32 x 8 tile and channel)"""
    return C * ((H + 7) // 8) * ((W + 31) // 32)


def psnr_lattice(N, C, H, W, seed=0, equal_sample=None):
    """a, b fp32 [N, C, H, W], multiples of 2^-8 in [0, 1] with a - b in 2^-8 {-7 .. 7}; sum_sq [N] int64 = sum ((a - b) 2^8)^2.
    Every squared error is a multiple of 2^-16 and the per-sample sum stays below 2^24 such units (asserted), so sums[n][0] must be
    exactly sum_sq / 65536 whatever the order of the additions.  ``equal_sample``: that sample has a == b."""
    rng = np.random.default_rng(seed)
    bi = rng.integers(0, 257, size=(N, C, H, W))
    ai = np.clip(bi + rng.integers(-7, 8, size=(N, C, H, W)), 0, 256)
    if equal_sample is not None:
        ai[equal_sample] = bi[equal_sample]
    d = ai - bi
    assert np.abs(d).max() <= 7
    assert C * H * W * 49 < FP32_EXACT, f"{C}x{H}x{W}: {C * H * W * 49} units of 2^-16 reach 2^24: the sum of squares is not order-free"
    return (ai / 256.0).astype(np.float32), (bi / 256.0).astype(np.float32), (d * d).reshape(N, -1).sum(1)


def psnr_from_sum_sq(sum_sq, count):
    with np.errstate(divide="ignore"):
        return 10 * np.log10(count * 65536.0 / np.asarray(sum_sq, np.float64))


def ssim_pair(family, N, C, H, W, seed=0):
    """'noise': rand, and rand + 0.05 randn clamped to [0, 1].  'smooth': a product of sinusoids (a different frequency and phase per
    plane), and the same + 0.01 randn clamped.  (Near-constant pairs are left out on purpose: there the cancellation E[x^2] - mu^2 against
    C2 = 9e-4 moves ANY fp32 evaluation by up to 9e-6, which says nothing about a kernel; slower sinusoids than these -- 0.21 / 0.13
    rad per pixel -- already move it by 2.7e-6.)"""
    gen = torch.Generator().manual_seed(seed)
    if family == "noise":
        a = torch.rand(N, C, H, W, generator=gen)
        b = (a + 0.05 * torch.randn(N, C, H, W, generator=gen)).clamp(0, 1)
    else:
        assert family == "smooth"
        y = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
        x = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
        k = torch.arange(N * C, dtype=torch.float64).view(N, C, 1, 1)
        a = (0.5 + 0.4 * torch.sin(0.6 * y + 0.7 * k) * torch.sin(0.5 * x + 0.3 + 0.4 * k)).float()
        b = (a + 0.01 * torch.randn(N, C, H, W, generator=gen)).clamp(0, 1)
    return a.numpy(), b.numpy()


# ------------------------------------------------------------------------------------------- Gaussian blur kernels

def ref_gaussian_kernels(params, K):
    """[N, K, K] fp64 from fp32 params [N, 3] = (sigma_x, sigma_y, theta [rad])"""
    params = np.asarray(params)
    assert params.dtype == np.float32
    r = int(K / 2)
    rng_ = np.linspace(-r, r, K).reshape(1, -1)
    xx, yy = np.tile(rng_, (K, 1)), np.tile(rng_.T, (1, K))
    out = np.empty((len(params), K, K), np.float64)
    for n, (sx, sy, th) in enumerate(params.astype(np.float64)):
        ct, st = np.cos(th), np.sin(th)
        sx2, sy2 = 2.0 * sx ** 2, 2.0 * sy ** 2
        a = ct ** 2 / sx2 + st ** 2 / sy2
        b = st * ct * (1.0 / sy2 - 1.0 / sx2)
        c = st ** 2 / sx2 + ct ** 2 / sy2
        k = np.exp(-(a * xx ** 2 + 2.0 * b * xx * yy + c * yy ** 2))
        out[n] = k / k.sum()
    return out


GAUSS_K = [1, 2, 3, 21, 22, 31]
GAUSS_CORNERS = np.asarray([(0.2, 0.2, 0.0), (0.2, 4.0, math.pi / 2), (0.2, 4.0, math.pi), (4.0, 4.0, 1.0), (4.0, 0.2, 0.3)], np.float32)


# ------------------------------------------------------------------------------------------- chunked loss reductions

L1_SHAPE = (2, 3, 181 * 123)          # N, C, hw: C * hw = 66789 = two chunks of 33395, the boundary inside plane 1
PLANE_SHAPE = (3, 66065)              # planes, hw: two chunks of 33033
SEG_SHAPE = (2, 365, 181)             # N, H, W: hw = 66065


def l1_lattice(seed=0):
    """dict for csbsr_l1_fwd_bwd at L1_SHAPE: a, b [N, C, hw] multiples of 2^-8 with a - b in 2^-8 {-15 .. 15} (a quarter of them 0),
    wmap [N, hw] in 2^-2 {2 .. 6}, power-of-two gscale / gs_n, a previous gradient da0 on 2^-4, and the exact results: sums_w / sums_1
    [N] (with / without wmap) and the gradients da_w / da_1 (stored) -- add da0 for the accumulate path.  The terms w |a - b| are
    multiples of 2^-10 and their per-sample total stays below 2^24 units (asserted)."""
    rng = np.random.default_rng(seed)
    N, C, hw = L1_SHAPE
    bi = rng.integers(0, 257, size=(N, C, hw))
    d = rng.integers(-15, 16, size=(N, C, hw)) * (rng.random((N, C, hw)) < 0.75)
    wi = rng.integers(2, 7, size=(N, 1, hw))
    assert int((wi * np.abs(d)).reshape(N, -1).sum(1).max()) < FP32_EXACT and 6 * 15 * C * hw < FP32_EXACT
    assert (d == 0).sum() > 1000
    gscale, gs_n = 0.5, np.asarray([2.0, 0.25], np.float32)
    sign = np.sign(d).astype(np.float64)
    scale = gscale * gs_n.astype(np.float64).reshape(N, 1, 1)
    out = dict(a=((bi + d) / 256.0).astype(np.float32), b=(bi / 256.0).astype(np.float32), wmap=(wi[:, 0] / 4.0).astype(np.float32),
               gscale=gscale, gs_n=gs_n, da0=(rng.integers(-32, 33, size=(N, C, hw)) / 16.0).astype(np.float32),
               sums_w=((wi * np.abs(d)).reshape(N, -1).sum(1) / 1024.0).astype(np.float32),
               sums_1=(np.abs(d).reshape(N, -1).sum(1) / 256.0).astype(np.float32),
               da_w=(scale * (wi / 4.0) * sign).astype(np.float32), da_1=(scale * sign).astype(np.float32))
    assert np.array_equal(out["a"].astype(np.float64) - out["b"].astype(np.float64), d / 256.0)      # a - b is exact in fp32 too
    return out


def plane_lattice(seed=0):
    """a, b fp32 [planes, hw] in 2^-8 {0 .. 12} and the exact sums: sum_a, sum_aa, sum_ab [planes] (fp32-exact: the sums of squares
    stay below 2^24 units of 2^-16, asserted)"""
    rng = np.random.default_rng(seed)
    planes, hw = PLANE_SHAPE
    ai, bi = rng.integers(0, 13, size=(planes, hw)), rng.integers(0, 13, size=(planes, hw))
    assert 144 * hw < FP32_EXACT
    return dict(a=(ai / 256.0).astype(np.float32), b=(bi / 256.0).astype(np.float32), sum_a=(ai.sum(1) / 256.0).astype(np.float32),
                sum_aa=((ai * ai).sum(1) / 65536.0).astype(np.float32), sum_ab=((ai * bi).sum(1) / 65536.0).astype(np.float32))


def segloss_inputs(seed=0):
    """p [N, 1, H, W] in [0, 1) with a run of exact zeros (the clamp at 1e-8), t {0, 1} -- sample 1 has an EMPTY target -- as fp32
    torch tensors; the signed distance map comes from the oracle in the test"""
    gen = torch.Generator().manual_seed(seed)
    N, H, W = SEG_SHAPE
    p = torch.rand(N, 1, H, W, generator=gen)
    p[0, 0, 0, :7] = 0.0
    p[1, 0, 182, 90:97] = 0.0             # flat index 33032 .. 33038: either side of the chunk boundary at 33033
    t = (torch.rand(N, 1, H, W, generator=gen) > 0.8).float()
    t[1] = 0.0
    return p, t


# ------------------------------------------------------------------------------------------- entry points and their rows

# rows (test ids of tests/test_metrics_exact_gpu.py) per C entry point: all of csrc/data_ops.hip, and the loss reductions that share
# its 65536-element chunk rule
LOSS_ENTRY_POINTS = {"csbsr_l1_fwd_bwd": "image_ops.hip", "csbsr_segloss_reduce": "image_ops.hip", "csbsr_segloss_finish": "image_ops.hip",
                     "csbsr_plane_reduce": "elementwise.hip"}
CASES = {
    "csbsr_iou_sweep": ["test_iou_counts_exact", "test_iou_threshold_counts", "test_iou_all_background_sample", "test_iou_refuses_1025_thresholds"],
    "csbsr_psnr_ssim": ["test_psnr_exact", "test_ssim_fp64"],
    "csbsr_gaussian_kernels": ["test_gaussian_kernels"],
    "csbsr_l1_fwd_bwd": ["test_l1_two_chunks_exact"],
    "csbsr_plane_reduce": ["test_plane_reduce_two_chunks_exact"],
    "csbsr_segloss_reduce": ["test_segloss_two_chunks"],
    "csbsr_segloss_finish": ["test_segloss_two_chunks"],
}
NOT_COVERED = {}          # entry point -> the written reason (six words at least) why it has no row


def data_ops_entry_points(text=None):
    if text is None:
        with open(os.path.join(CSRC, "data_ops.hip")) as f:
            text = f.read()
    return re.findall(r'extern "C" int (csbsr_\w+)', text)


def missing_entry_points(cases, not_covered, names=None):
    """the entry points of data_ops.hip and the chunked loss reductions with neither a row nor a reason"""
    names = data_ops_entry_points() + list(LOSS_ENTRY_POINTS) if names is None else names
    return [n for n in names if not cases.get(n) and n not in not_covered]
