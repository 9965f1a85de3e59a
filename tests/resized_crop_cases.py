"""Shared by the resized-crop tests and tests/golden/make_resized_crop_golden.py: the NumPy restatement of csbsr_gather_resize_u8
(include/csbsr_hip.h) in fp64 and fp32 with border clamp and flips, torchvision's published RandomResizedCrop.get_params restated over
given uniforms, and the case lists.  No GPU, no reference code."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resized_crop_batch.npz")
CROP = (16, 24)
SIZES = [(29, 40), (16, 24), (33, 27), (21, 47), (38, 31), (17, 52), (26, 36), (31, 25)]       # those of make_resident_golden.py
BIG = (130, 200)
PARITY_SIZES = SIZES + [BIG]
TWO_POW_M24 = 2.0 ** -24


# --------------------------------------------------------------------------------------------------------------- the resample
def axis_weights(n_in, n_out, antialias, dt):
    """[(first source index, normalised weights)] per output index, every step in the precision ``dt``."""
    scale = dt(n_in) / dt(n_out)
    shrink = bool(antialias) and scale >= 1
    support = scale if shrink else dt(1.0)
    inv = dt(1.0) / scale if shrink else dt(1.0)
    out = []
    for o in range(n_out):
        c = scale * dt(o + 0.5)
        lo = max(0, int(c - support + dt(0.5)))
        hi = min(n_in, int(c + support + dt(0.5)))
        wt = [max(dt(0), dt(1) - abs((dt(j) - c + dt(0.5)) * inv)) for j in range(lo, hi)]
        total = dt(0)
        for v in wt:
            total = total + v                  # in ascending order, as the kernel and torch add them
        out.append((lo, np.array([v / total for v in wt], dtype=dt)))
    return out


def resize_window(win, h, w, antialias, dt):
    """win [C][hs][ws] (any real dtype) -> [C][h][w] in ``dt``: horizontal pass first, taps added in ascending order."""
    C, hs, ws = win.shape
    a = win.astype(dt)
    t = np.zeros((C, hs, w), dt)
    for o, (x0, k) in enumerate(axis_weights(ws, w, antialias, dt)):
        acc = np.zeros((C, hs), dt)
        for i, kk in enumerate(k):
            acc = acc + kk * a[:, :, x0 + i]
        t[:, :, o] = acc
    r = np.zeros((C, h, w), dt)
    for o, (y0, k) in enumerate(axis_weights(hs, h, antialias, dt)):
        acc = np.zeros((C, w), dt)
        for i, kk in enumerate(k):
            acc = acc + kk * t[:, y0 + i, :]
        r[:, o, :] = acc
    return r


def window_of(a, row):
    """uint8 H x W x C (or H x W), row (index, y0, x0, mirror, vflip, hs, ws) -> uint8 [C][hs][ws]: flips on the whole image, then the
    window, its coordinates clamped into the image (border replication for a window that overhangs)."""
    _, y0, x0, mirror, vflip, hs, ws = (int(v) for v in row)
    if a.ndim == 2:
        a = a[:, :, None]
    if mirror:
        a = a[:, ::-1]
    if vflip:
        a = a[::-1]
    ys = np.clip(np.arange(y0, y0 + hs), 0, a.shape[0] - 1)
    xs = np.clip(np.arange(x0, x0 + ws), 0, a.shape[1] - 1)
    return np.ascontiguousarray(a[ys][:, xs].transpose(2, 0, 1))


def gather_resize_numpy(arrays, sel7, h, w, antialias, dt):
    """arrays: list of uint8 images; sel7 [B][7] -> [B][C][h][w] in ``dt``, divided by 255 in ``dt``."""
    return np.stack([resize_window(window_of(arrays[int(r[0])], r), h, w, antialias, dt) / dt(255) for r in np.asarray(sel7)])


def gather_resize_torch(arrays, sel7, h, w, antialias):
    """The same through torch's CPU F.interpolate in fp32: what the reference's resized_crop evaluates."""
    import torch
    import torch.nn.functional as F
    out = []
    for r in np.asarray(sel7):
        win = torch.from_numpy(window_of(arrays[int(r[0])], r).astype(np.float32))[None]
        out.append((F.interpolate(win, size=(h, w), mode="bilinear", align_corners=False, antialias=bool(antialias))[0] / 255).numpy())
    return np.stack(out)


def tolerance(arrays, sel7, h, w, antialias):
    """(fp64 restatement, bound): bound = 2 * max|torch CPU fp32 - fp64 restatement| + 2^-24 for this case."""
    r64 = gather_resize_numpy(arrays, sel7, h, w, antialias, np.float64)
    e_ref = float(np.abs(gather_resize_torch(arrays, sel7, h, w, antialias).astype(np.float64) - r64).max())
    return r64, e_ref, 2 * e_ref + TWO_POW_M24


# --------------------------------------------------------------------------------------------------------------- the window draw
def get_params(H, W, scale, ratio, u_tries, u_off):
    """torchvision's RandomResizedCrop.get_params over given uniforms: u_tries [10][2] = (area, aspect) per try, u_off = (y, x).
    -> (y0, x0, hs, ws, took): ``took`` False for the central fallback."""
    area = H * W
    for ua, ur in u_tries:
        t = area * (scale[0] + (scale[1] - scale[0]) * ua)
        r = math.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * ur)
        ws, hs = int(round(math.sqrt(t * r))), int(round(math.sqrt(t / r)))
        if 0 < ws <= W and 0 < hs <= H:
            return min(int(u_off[0] * (H - hs + 1)), H - hs), min(int(u_off[1] * (W - ws + 1)), W - ws), hs, ws, True
    if W / H < ratio[0]:
        ws, hs = W, int(round(W / ratio[0]))
    elif W / H > ratio[1]:
        hs, ws = H, int(round(H * ratio[1]))
    else:
        hs, ws = H, W
    return (H - hs) // 2, (W - ws) // 2, hs, ws, False


# --------------------------------------------------------------------------------------------------------------- inputs and cases
def parity_inputs(seed=20241018):
    """uint8 images of PARITY_SIZES (every byte value) and masks with arbitrary bytes (a JPEG mask is not {0, 255})."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for H, W in PARITY_SIZES]
    masks = [rng.integers(0, 256, size=(H, W), dtype=np.uint8) for H, W in PARITY_SIZES]
    return images, masks


def parity_rows():
    """B = 12 rows (index, y0, x0, mirror, vflip, hs, ws), a different window per sample: a full image 29x40, 38x31 (2.4x / 1.3x down),
    9x13 (up), 1x1, 127x190 (just under the 8x cap of output (16, 24)), 40x9 (down in y, up in x), windows touching each edge, flips."""
    rows = [
        (0, 0, 0, 0, 0, 29, 40),          # a full image
        (4, 0, 0, 1, 0, 38, 31),          # a full image, 2.4x / 1.3x down, mirrored
        (2, 5, 3, 0, 1, 9, 13),           # up, flipped
        (3, 20, 46, 1, 1, 1, 1),          # one pixel, the last of its image, both flips
        (8, 3, 10, 0, 0, 127, 190),       # just under the cap, touches the bottom and the right edge
        (8, 0, 0, 1, 1, 127, 190),        # the same size at the top left, both flips
        (8, 45, 100, 0, 1, 40, 9),        # down in y, up in x
        (5, 0, 12, 0, 0, 17, 30),         # touches top and bottom
        (6, 3, 0, 1, 0, 20, 21),          # touches the left edge (of the mirrored image)
        (7, 11, 8, 0, 1, 20, 17),         # touches the bottom and the right edge
        (1, 0, 0, 1, 1, 16, 24),          # an image of the output size: the identity
        (3, 2, 7, 0, 0, 16, 33),          # identity in y, 1.4x down in x
    ]
    return np.array(rows, dtype=np.int32)


def parity_rows_for(h, w):
    """parity_rows with the two windows over the 8x cap of a smaller output cut down to just under it."""
    rows = parity_rows().copy()
    rows[:, 5] = np.minimum(rows[:, 5], 8 * h - 1)
    rows[:, 6] = np.minimum(rows[:, 6], 8 * w - 1)
    return rows


def wide_rows():
    """windows of about 93 x 301 on an image of 130 x 330 for output (40, 136): more than one workgroup tile in both directions"""
    return np.array([(0, 20, 10, 0, 0, 93, 301), (0, 37, 29, 1, 1, 93, 301), (0, 0, 0, 1, 0, 91, 299), (0, 30, 20, 0, 1, 100, 310)], dtype=np.int32)


WIDE_SIZE, WIDE_OUT = (130, 330), (40, 136)
ODD_OUT = (10, 18)                                          # w % 4 != 0: the per-element tail


def wide_inputs(seed=5):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=WIDE_SIZE + (3,), dtype=np.uint8)], [rng.integers(0, 256, size=WIDE_SIZE, dtype=np.uint8)]


# (images H x W, window rows) with the window hanging over the image by 1 .. 3 pixels on each side
CLAMP_SIZE = (20, 28)
CLAMP_ROWS = np.array([(1, -1, -2, 0, 0, 24, 33), (1, -3, -1, 1, 0, 26, 30), (1, -2, -3, 0, 1, 23, 34), (1, 5, 20, 1, 1, 18, 11),
                       (1, -1, 4, 0, 0, 16, 24)], dtype=np.int32)


def load_golden():
    z = np.load(GOLDEN)
    n = int(z["n_images"])
    return {"images": [z[f"image_{i}"] for i in range(n)], "masks": [z[f"mask_{i}"] for i in range(n)], "sel": z["sel"],
            "crop": tuple(int(v) for v in z["crop"]), "out_image": z["out_image"], "out_mask": z["out_mask"]}
