"""Tolerance-matched precision / recall counts (csrc/pr_sweep.hip, utils/estimate_metrics.pr_sweep) restated in NumPy, twice, and the
cases of tests/test_pr_sweep_cpu.py and tests/test_pr_sweep_gpu.py.

``counts_per_threshold`` is the definition: for every threshold its own binary map, two Euclidean distance transforms (SciPy) and "match
iff the rounded squared distance is <= tol2".  ``counts_histogram`` is the one-pass form the kernel takes: one level plane, the disk's
dilation of the gt plane (near), the disk's maximum of the level plane (m), three histograms and their suffix sums.  The CPU test holds
the two equal on every case; the GPU tests then ask the device for exact integer equality.

A case is (pred [N,H,W] fp32, mask [N,H,W] fp32, thresholds (list of floats), tol2).  The kernel's tiles are 32 rows by 64 columns, so the
seams lie at y = 32 and x = 64, 128; the sizes 37 x 70 and 33 x 129 leave a remainder of a few pixels behind each seam."""
import csv
import functools

import numpy as np

THRESHOLDS = [i * 0.01 for i in range(1, 100)]            # the project's sweep
TH1 = [0.5]
TH255 = [(i + 1) / 256 for i in range(255)]
TOL2 = (0, 1, 2, 4, 5, 25, 256)
SEAM_Y, SEAM_X = 32, 64


def th32(thresholds):
    return np.array([float(t) for t in thresholds], dtype=np.float32)


def levels(pred, t32):
    """number of thresholds j with pred - t_j > 0 in fp32 (NaN -> 0), as an int64 plane"""
    with np.errstate(invalid="ignore"):
        return ((pred[None].astype(np.float32) - t32.reshape(-1, *([1] * pred.ndim))) > 0).sum(0)


def disk(tol2):
    r = int(np.floor(np.sqrt(tol2)))
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= tol2]


# ------------------------------------------------------------------------------------------------------------ the definition
def _d2_to(binary):
    """rounded squared distance of every pixel to the nearest set pixel of ``binary`` (int64); None when nothing is set"""
    from scipy.ndimage import distance_transform_edt
    if not binary.any():
        return None
    d = distance_transform_edt(~binary)
    return np.rint(d * d).astype(np.int64)


def counts_per_threshold(pred, mask, thresholds, tol2):
    """int64 [N, 4, T] = (n_pred, tp_pred, tp_gt, n_gt), one binary map and one distance transform per threshold."""
    t32 = th32(thresholds)
    N, T = pred.shape[0], len(t32)
    out = np.zeros((N, 4, T), np.int64)
    for n in range(N):
        gt = mask[n] > np.float32(0.5)
        d2_gt = _d2_to(gt)                                # the gt map does not change with the threshold
        for j in range(T):
            with np.errstate(invalid="ignore"):
                p = (pred[n] - t32[j]) > 0
            d2_p = _d2_to(p)
            out[n, 0, j] = p.sum()
            out[n, 1, j] = 0 if d2_gt is None else (p & (d2_gt <= tol2)).sum()
            out[n, 2, j] = 0 if d2_p is None else (gt & (d2_p <= tol2)).sum()
            out[n, 3, j] = gt.sum()
    return out


# ------------------------------------------------------------------------------------------------------------ the one-pass form
def counts_histogram(pred, mask, thresholds, tol2):
    """int64 [N, 4, T] from the level plane alone: near = any gt in p + D, m = max level in p + D (zero outside the image),
    n_pred[j] = #{level > j}, tp_pred[j] = #{level > j and near}, tp_gt[j] = #{gt and m > j}, n_gt = #gt."""
    t32 = th32(thresholds)
    N, T = pred.shape[0], len(t32)
    H, W = pred.shape[1:]
    r = int(np.floor(np.sqrt(tol2)))
    out = np.zeros((N, 4, T), np.int64)
    for n in range(N):
        lv = levels(pred[n], t32)
        gt = mask[n] > np.float32(0.5)
        lp, gp = np.pad(lv, r), np.pad(gt, r)
        near, m = np.zeros((H, W), bool), np.zeros((H, W), np.int64)
        for dy, dx in disk(tol2):
            near |= gp[r + dy:r + dy + H, r + dx:r + dx + W]
            m = np.maximum(m, lp[r + dy:r + dy + H, r + dx:r + dx + W])
        h_all = np.bincount(lv.reshape(-1), minlength=T + 1)
        h_near = np.bincount(lv[near], minlength=T + 1)
        h_gt = np.bincount(m[gt], minlength=T + 1)
        suffix = lambda h: np.cumsum(h[::-1])[::-1][1:]   # [j] = sum of the bins above j
        out[n] = np.stack([suffix(h_all), suffix(h_near), suffix(h_gt), np.full(T, gt.sum())])
    return out


# ------------------------------------------------------------------------------------------------------------ inputs
def make_image(seed, H, W, thresholds=THRESHOLDS, special=True):
    """(pred, mask) fp32 [H, W].  mask: thin cracks on all four borders and across every tile seam, a diagonal, soft values 0.5 (not gt) and
    0.51 (gt).  pred: a low background (level 0) with blobs and strokes one to three pixels off the cracks, on the borders and across the
    seams too; with ``special`` also values equal to a threshold in fp32, their fp32 neighbours, NaN, +-inf, values <= 0 and > 1."""
    rng = np.random.default_rng(seed)
    t32 = th32(thresholds)
    mask = np.zeros((H, W), np.float32)
    pred = (rng.random((H, W)) * 0.009).astype(np.float32)                  # below every threshold of the project's sweep
    if H >= 8 and W >= 8:
        mask[0, W // 4:W // 2] = 1                                          # the four borders
        mask[H - 1, W // 3:] = 1
        mask[H // 4:, 0] = 1
        mask[:H // 2, W - 1] = 1
        for sx in range(SEAM_X, W, SEAM_X):                                 # a horizontal crack through every vertical seam
            mask[H // 2, max(0, sx - 5):sx + 4] = 1
        if H > SEAM_Y:
            mask[SEAM_Y - 3:min(H, SEAM_Y + 3), W // 5] = 1                 # a vertical crack through the horizontal seam
        for i in range(min(H, W) - 6):                                      # a diagonal
            mask[3 + i, 3 + i] = 1
        yy, xx = np.nonzero(mask)
        for off, val in (((1, 0), 0.9), ((0, 2), 0.6), ((-2, 1), 0.35), ((3, 0), 0.2)):      # the cracks again, off centre and fainter
            sel = rng.random(len(yy)) < 0.6
            y, x = np.clip(yy[sel] + off[0], 0, H - 1), np.clip(xx[sel] + off[1], 0, W - 1)
            pred[y, x] = np.maximum(pred[y, x], (val * rng.random(sel.sum())).astype(np.float32))
        for _ in range(4):                                                  # blobs, some of them far from any crack, some on a seam
            y, x, s = int(rng.integers(0, H)), int(rng.integers(0, W)), int(rng.integers(1, 4))
            pred[max(0, y - s):y + s + 1, max(0, x - s):x + s + 1] = rng.random()
        pred[max(0, SEAM_Y - 2):SEAM_Y + 2, max(0, min(W, SEAM_X) - 2):SEAM_X + 2] = 0.77
        pred[0, :3], pred[H - 1, W - 3:], pred[H - 3:, 0], pred[:3, W - 1] = 0.95, 0.85, 0.75, 0.65      # the corners
        soft = rng.random((H, W))
        mask[(soft < 0.01) & (mask == 0)] = 0.5                             # not gt
        mask[(soft > 0.99) & (mask == 0)] = 0.51                            # gt
    else:
        pred[:] = rng.random((H, W)).astype(np.float32)
        mask[:] = (rng.random((H, W)) < 0.5).astype(np.float32)
    if special and H * W >= 64:
        flat = pred.reshape(-1)
        free = np.ones((H, W), bool)                                        # the seam block and the corners keep their values
        free[max(0, SEAM_Y - 2):SEAM_Y + 2, max(0, min(W, SEAM_X) - 2):SEAM_X + 2] = False
        free[0, :3], free[H - 1, W - 3:], free[H - 3:, 0], free[:3, W - 1] = False, False, False, False
        idx = rng.choice(np.flatnonzero(free), size=min(H * W // 2, 3 * len(t32) + 8), replace=False)
        vals = np.concatenate([t32, np.nextafter(t32, np.float32(2)), np.nextafter(t32, np.float32(-1)),
                               np.array([np.nan, np.nan, np.inf, -np.inf, 0.0, -0.25, 1.0, 1.5], np.float32)])
        flat[idx] = vals[:len(idx)]
    return pred, mask


# (dy, dx) with dy^2 + dx^2 = tol2, and the same for the smallest sum of two squares above tol2 (tol2 + 1 where that is one: 3 and 6 are not)
EXACT = {0: (0, 0), 1: (0, 1), 2: (1, 1), 4: (0, 2), 5: (1, 2), 25: (3, 4), 256: (0, 16)}
BEYOND = {0: (0, 1), 1: (1, 1), 2: (0, 2), 4: (1, 2), 5: (2, 2), 25: (1, 5), 256: (1, 16)}


def boundary_pair(tol2):
    """40 x 200, one threshold (0.5): a gt pixel at (31, 63) and a predicted pixel at squared distance exactly tol2 from it, on the far side
    of the seam x = 64 (and of y = 32 where dy > 0); a second pair at (31, 127) at the smallest squared distance above tol2, across x = 128.
    The first pair matches, the second does not: counts = (2, 1, 1, 2)."""
    pred, mask = np.zeros((1, 40, 200), np.float32), np.zeros((1, 40, 200), np.float32)
    for (gy, gx), (dy, dx) in (((31, 63), EXACT[tol2]), ((31, 127), BEYOND[tol2])):
        mask[0, gy, gx] = 1
        pred[0, gy + dy, gx + dx] = 1
    return pred, mask, TH1, tol2


def _stack(*imgs):
    return np.stack([p for p, _ in imgs]), np.stack([m for _, m in imgs])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (pred [N,H,W], mask [N,H,W], thresholds, tol2), built once; nothing mutates them."""
    c = {}
    for H, W in ((37, 70), (33, 129)):
        for tol2 in TOL2:
            c[f"{H}x{W}_tol2_{tol2}"] = _stack(make_image(H * W + tol2, H, W)) + (THRESHOLDS, tol2)
    one, zero = np.ones((1, 1, 1), np.float32), np.zeros((1, 1, 1), np.float32)
    for tag, p, m in (("hit", one, one), ("miss", one, zero), ("none", zero, one)):
        for tol2 in (0, 4):
            c[f"1x1_{tag}_tol2_{tol2}"] = (p, m, TH1, tol2)
    c["9x9_tol2_256"] = _stack(make_image(9, 9, 9)) + (THRESHOLDS, 256)                   # the disk is larger than the image
    for tol2 in TOL2:
        c[f"boundary_tol2_{tol2}"] = boundary_pair(tol2)
    p, m = _stack(make_image(5, 37, 70))
    c["empty_gt"] = (p, np.zeros_like(m), THRESHOLDS, 4)
    c["empty_pred"] = (np.zeros_like(p), m, THRESHOLDS, 4)
    c["ones_pred"] = (np.ones_like(p), m, THRESHOLDS, 4)
    c["ones_mask"] = (p, np.ones_like(m), THRESHOLDS, 4)
    c["T1"] = _stack(make_image(6, 37, 70, TH1)) + (TH1, 5)
    c["T255"] = _stack(make_image(7, 37, 70, TH255)) + (TH255, 5)
    c["batch3"] = _stack(make_image(8, 33, 129), make_image(9, 33, 129), make_image(10, 33, 129, special=False)) + (THRESHOLDS, 4)
    return c


@functools.lru_cache(maxsize=None)
def realistic():
    """(pred, mask [2, 448, 448], THRESHOLDS, tol2 = 4): synthetic crack masks (csbsr_amd/data/synthetic.py) and smooth model-like maps --
    the mask moved one or two pixels off centre, blurred, plus faint smooth clutter."""
    import torch
    from scipy.ndimage import gaussian_filter
    from csbsr_amd.data.synthetic import crack_masks
    mask = crack_masks(2, 448, 448, torch.Generator().manual_seed(448))[:, 0].numpy().astype(np.float32)
    rng = np.random.default_rng(448)
    pred = np.empty_like(mask)
    for n, shift in enumerate(((1, 2), (-2, 1))):
        blur = gaussian_filter(np.roll(mask[n], shift, axis=(0, 1)).astype(np.float64), 1.5 + n)
        clutter = gaussian_filter(rng.random((448, 448)), 6.0)
        pred[n] = np.clip(0.9 * blur / blur.max() + 0.6 * (clutter - clutter.mean()), 0, 1).astype(np.float32)
    return pred, mask, THRESHOLDS, 4


@functools.lru_cache(maxsize=None)
def realistic_reference():
    """the per-threshold SciPy form of ``realistic`` (2 x 99 distance transforms of 448 x 448), computed once per process"""
    return counts_per_threshold(*realistic())


# ------------------------------------------------------------------------------------------------------------ scores, naively
def scores_naive(counts):
    """precision, recall, f [N][T] as lists of Python floats, cell by cell, with the three conventions of inference.pr_scores"""
    out = ([], [], [])
    for img in np.asarray(counts).tolist():
        rows = ([], [], [])
        for n_pred, tp_pred, tp_gt, n_gt in zip(*img):
            p = tp_pred / n_pred if n_pred else 1.0
            r = tp_gt / n_gt if n_gt else 1.0
            f = 2.0 * p * r / (p + r) if p + r > 0 else 0.0
            for lst, v in zip(rows, (p, r, f)):
                lst.append(v)
        for o, lst in zip(out, rows):
            o.append(lst)
    return out


def summary_naive(counts, thresholds):
    c = np.asarray(counts, dtype=np.int64)
    total = [[int(c[:, k, j].sum()) for j in range(c.shape[2])] for k in range(4)]
    p, r, f = (a[0] for a in scores_naive([total]))
    best = max(range(len(f)), key=lambda j: (f[j], -j))                       # the first maximum
    ois = sum(max(row) for row in scores_naive(c)[2]) / c.shape[0]
    ap = 0.0
    for j in range(len(f) - 1):
        ap += (r[j] - r[j + 1]) * (p[j] + p[j + 1]) * 0.5
    return {"ODS": f[best], "ODS_threshold": float(thresholds[best]), "OIS": ois, "AP": ap, "P_at_ODS": p[best], "R_at_ODS": r[best]}


def read_pr_log(path):
    """(fnames, thresholds, precision, recall, f) of a pr_log.csv as inference.write_pr_log lays it out"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    thresholds = [float(t) for t in rows[0][2:]]
    fnames, vals = [], {"P": [], "R": [], "F": []}
    for row in rows[1:]:
        if row[1] == "P":
            fnames.append(row[0])
        vals[row[1]].append([float(v) for v in row[2:]])
    return (fnames, thresholds) + tuple(np.asarray(vals[k], dtype=np.float64).reshape(len(fnames), len(thresholds)) for k in "PRF")
