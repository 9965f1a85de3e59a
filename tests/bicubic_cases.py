"""What the MODEL.SR="bicubic" tests share: the fp64 NumPy restatement of torchvision's Resize(BICUBIC) on a float tensor for an integer
up-scale (both antialias settings), the kernel's case table, and a cached reader of the fixture.

Restatement, per axis, for output index o of n * s (c = (o + 0.5) / s):
  antialias=True   F.interpolate(bicubic, antialias=True): Keys' cubic with A = -0.5, taps j in [max(int(c - 1.5), 0), min(int(c + 2.5), n)),
                   w_j = cub(j - c + 0.5) divided by the sum of the tap weights -- the taps are CUT to the image and renormalised;
  antialias=False  F.interpolate(bicubic): A = -0.75, the four taps floor(c - 0.5) - 1 .. + 2 with their INDICES clamped to the image.
  cub(t) = ((A + 2)|t| - (A + 3)) t^2 + 1 for |t| <= 1,  A (((|t| - 5)|t| + 8)|t| - 4) for 1 < |t| < 2,  0 beyond;  y = M_y x M_x^T.
"""
import functools
import math

import numpy as np

# (planes, H, W, scale): every tap set cut at a border / odd sizes / scale 8 / several planes and more than one workgroup tile (256 x 16
# outputs) down a plane / more than one tile ALONG a row, the last one partly filled: 280 and 320 outputs per row (blockIdx.x >= 1)
KERNEL_CASES = [(3, 2, 3, 4), (6, 9, 7, 4), (3, 5, 6, 8), (12, 33, 17, 4), (2, 5, 70, 4), (2, 3, 40, 8)]


def cub(t, A):
    t = abs(t)
    if t <= 1.0:
        return ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0
    if t < 2.0:
        return A * (((t - 5.0) * t + 8.0) * t - 4.0)
    return 0.0


def up_matrix(n, s, antialias=True):
    """fp64 [n * s, n]: the axis operator of the up-scale"""
    M = np.zeros((n * s, n), dtype=np.float64)
    for o in range(n * s):
        c = (o + 0.5) / s
        if antialias:
            lo, hi = max(int(c - 1.5), 0), min(int(c + 2.5), n)
            w = np.array([cub(j - c + 0.5, -0.5) for j in range(lo, hi)], dtype=np.float64)
            M[o, lo:hi] = w / w.sum()
        else:
            f = math.floor(c - 0.5)
            t = c - 0.5 - f
            for k, wk in enumerate((cub(t + 1.0, -0.75), cub(t, -0.75), cub(1.0 - t, -0.75), cub(2.0 - t, -0.75))):
                M[o, min(max(f - 1 + k, 0), n - 1)] += wk
    return M


def bicubic_up_ref(x, s, antialias=True, clip=False):
    """fp64 [..., H * s, W * s] of an array [..., H, W]"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    y = np.einsum("oh,...hw,pw->...op", up_matrix(H, s, antialias), x, up_matrix(W, s, antialias))
    return np.clip(y, 0.0, 1.0) if clip else y


def case_input(planes, H, W, scale):
    """fp32 [planes, H, W] drawn from [-0.2, 1.2], so that the clip bites"""
    rng = np.random.default_rng(1000 * planes + 100 * H + 10 * W + scale)
    return (rng.random((planes, H, W)) * 1.4 - 0.2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_reference(planes, H, W, scale, antialias):
    """the restatement of a kernel case, computed once and shared (read-only)"""
    y = bicubic_up_ref(case_input(planes, H, W, scale), scale, bool(antialias))
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def fixture():
    """bicubic_pspnet.npz and bicubic_pspnet_eval.npz (the LR input, the BatchNorm buffers and the eval-mode outputs: one file would exceed 1 MiB) as one mapping"""
    from golden_utils import load_golden
    return {**load_golden("bicubic_pspnet"), **load_golden("bicubic_pspnet_eval")}
