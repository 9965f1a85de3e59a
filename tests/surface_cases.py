"""Shared by tests/test_surface_distance_{cpu,gpu}.py: the fixture tests/golden/surface_distance.npz (written by
tests/golden/make_surface_golden.py from the reference's surface_distance package) and a SciPy restatement of one (image, threshold) cell
of calc_distance_metrics: neighbour codes on the corner grid, scipy's EDT to the border corners, elements sorted ONE BY ONE by
(distance, length) as the reference sorts them.  The restatement takes the contour lengths from the fixture's table (the reference's
data), not from the code under test."""
import os

import numpy as np
from scipy import ndimage

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "surface_distance.npz")
MSD_RTOL = 1e-9          # both sides are fp64 sums of at most ~1e7 positive terms: |difference| <= n * eps relative


def load_fixture():
    return np.load(GOLDEN)


def fixture_inputs(g, name):
    """(prob fp32 [H,W] = k / 255, mask fp32 [H,W]) of one fixture case"""
    return g[f"prob_{name}"].astype(np.float32) / np.float32(255), g[f"mask_{name}"].astype(np.float32)


def binarise(prob32, thresholds):
    """[T,H,W] bool: segment_preds - torch.Tensor(thresholds) > 0 in fp32"""
    th = np.asarray([float(t) for t in thresholds], np.float32)
    return (prob32[None] - th[:, None, None]) > 0


def corner_codes(m):
    p = np.pad(np.asarray(m, bool).astype(np.int64), 1)
    return 8 * p[:-1, :-1] + 4 * p[:-1, 1:] + 2 * p[1:, :-1] + p[1:, 1:]


def _borders_and_maps(gt, pred):
    cg, cp = corner_codes(gt), corner_codes(pred)
    bg, bp = (cg != 0) & (cg != 15), (cp != 0) & (cp != 15)
    dg = ndimage.distance_transform_edt(~bg) if bg.any() else None
    dp = ndimage.distance_transform_edt(~bp) if bp.any() else None
    return cg, cp, bg, bp, dg, dp


def restate_cell(gt, pred, length_table, percent, max_img_len):
    """(hd, msd, hd_outlier, msd_outlier, margin) of one cell, element by element"""
    cg, cp, bg, bp, dg, dp = _borders_and_maps(gt, pred)
    if not bg.any() and not bp.any():
        return 0.0, 0.0, 0, 0, np.inf
    if not bg.any() or not bp.any():
        return float(max_img_len), float(max_img_len), 1, 1, np.inf
    perc, avg, margin = [], [], np.inf
    for d, a in ((dp[bg], length_table[cg[bg]]), (dg[bp], length_table[cp[bp]])):
        order = np.lexsort((a, d))
        d, a = d[order], a[order]
        cum = np.cumsum(a) / np.sum(a)
        perc.append(d[min(int(np.searchsorted(cum, percent / 100.0)), len(d) - 1)])
        avg.append(np.sum(d * a) / np.sum(a))
        margin = min(margin, float(np.min(np.abs(cum - percent / 100.0))))
    return float(max(perc)), float(avg[0] + avg[1]) / 2, 0, 0, margin


def integer_counts(gt, pred, class_table):
    """((keys, counts) gt -> pred, (keys, counts) pred -> gt), keys = d^2 * 4 + class, from scipy's EDT; empty where a contour is missing"""
    cg, cp, bg, bp, dg, dp = _borders_and_maps(gt, pred)
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    if not bg.any() or not bp.any():
        one = (np.zeros(1, np.int64), np.ones(1, np.int64))          # the finish only asks whether a side is empty
        return (one if bg.any() else empty), (one if bp.any() else empty)
    out = []
    for d, c in ((dp[bg], cg[bg]), (dg[bp], cp[bp])):
        d2 = np.rint(d * d).astype(np.int64)
        assert np.array_equal(np.sqrt(d2.astype(np.float64)), d)     # scipy's distances are square roots of integers
        out.append(np.unique(d2 * 4 + class_table[c], return_counts=True))
    return out[0], out[1]


def compare_case(name, hd, msd, ref_hd, ref_msd, margin, tie_margin):
    """the acceptance rule: HD equal on every cell outside a percentile tie, MSD within MSD_RTOL relative (degenerate cells exactly)"""
    live = np.asarray(margin) >= tie_margin
    bad = np.nonzero(live & (hd != ref_hd))[0]
    assert bad.size == 0, f"{name}: HD differs at thresholds {bad[:8]}: {hd[bad][:8]} vs {ref_hd[bad][:8]}"
    err = np.abs(msd - ref_msd) / np.maximum(np.abs(ref_msd), 1e-300)
    err[ref_msd == msd] = 0
    assert err.max() <= MSD_RTOL, f"{name}: MSD rel err {err.max():.3e} at threshold {int(err.argmax())}"
    degenerate = ~np.isfinite(margin)
    assert np.array_equal(hd[degenerate], ref_hd[degenerate]) and np.array_equal(msd[degenerate], ref_msd[degenerate]), name
    return float(err.max()), int((~live).sum())
