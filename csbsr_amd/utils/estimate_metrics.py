"""Evaluation metrics on the device: PSNR, SSIM and the IoU threshold sweep of
model/utils/estimate_metrics.py:64-191 and model/engine/inference.py:50-53,111-119, as single-pass HIP kernels
(csbsr_psnr_ssim, csbsr_iou_sweep) instead of five depthwise convolutions per SSIM and a [B,99,H,W] broadcast + a host numpy
reduction per batch.  Same class names / call conventions as the reference; results come back as numpy arrays like there."""

import math

import numpy as np
import torch

from .. import _lib as L
from ..engine import _ptr, _reduction_scratch


def _dev32(t, like=None):
    dev = like.device if like is not None and like.is_cuda else (t.device if t.is_cuda else torch.device("cuda:0"))
    return t.to(dev, torch.float32).contiguous()


def psnr_ssim(img1, img2):
    """per-sample (PSNR [B], SSIM [B]) fp32 device tensors of two [B,C,H,W] batches in [0,1]."""
    L.load()
    a = _dev32(img1)
    b = _dev32(img2, a)
    B, Cc, H, W = a.shape
    _reduction_scratch(a.device)         # the sums are an order-fixed fold of per-workgroup partial rows (csrc/common.h)
    sums = torch.zeros(B, 2, dtype=torch.float32, device=a.device)
    ps, ss = torch.empty(B, dtype=torch.float32, device=a.device), torch.empty(B, dtype=torch.float32, device=a.device)
    L.call("csbsr_psnr_ssim", _ptr(a), _ptr(b), B, Cc, H, W, _ptr(sums), _ptr(ps), _ptr(ss), L.stream(a.device))
    return ps, ss


class PSNR:
    """estimate_metrics.py:89-101: 10 log10(1 / mse), batch dim retained, images in [0,1]."""
    name = "PSNR"

    def __call__(self, img1, img2):
        return psnr_ssim(img1, img2)[0].cpu().numpy().copy()


class SSIM:
    """estimate_metrics.py:164-191 (window 11, sigma 1.5, size_average=False: one value per sample)."""
    name = "SSIM"

    def __init__(self, window_size=11, size_average=False):
        if window_size != 11 or size_average:
            raise NotImplementedError("the device SSIM is built for the evaluation loop's setting: window 11, per-sample values")

    def __call__(self, img1, img2):
        return psnr_ssim(img1, img2)[1].cpu().numpy().copy()


def iou_sweep(segment_preds, masks, thresholds, smooth=1e-5):
    """IoU of (segment_preds - t > 0) vs (masks > 0.5) for every threshold: [B, len(thresholds)] fp32 device tensor
    (inference.py:111-119 with estimate_metrics.IoU)."""
    L.load()
    p = _dev32(segment_preds)
    m = _dev32(masks, p)
    B = p.shape[0]
    hw = p[0].numel()
    th = torch.tensor([float(t) for t in thresholds], dtype=torch.float32)          # == torch.Tensor(thresholds): fp32 roundings
    assert bool((th[1:] > th[:-1]).all()), "thresholds must ascend"
    th = th.to(p.device)
    T = th.numel()
    hist = torch.zeros(B, 2, T + 1, dtype=torch.int32, device=p.device)
    out = torch.empty(B, T, dtype=torch.float32, device=p.device)
    L.call("csbsr_iou_sweep", _ptr(p), _ptr(m), _ptr(th), B, hw, T, float(smooth), _ptr(hist), _ptr(out), None, None, L.stream(p.device))
    return out


PR_MAX_TOLERANCE = 16.0


def pr_tol2(tolerance):
    """squared radius of the matching disk: floor(tolerance^2) for a radius of 0 .. 16 pixels (2.0 -> 4); anything else is a ValueError."""
    t = float(tolerance)
    if not 0.0 <= t <= PR_MAX_TOLERANCE:              # NaN fails both comparisons
        raise ValueError(f"the matching tolerance is a radius of 0 .. {PR_MAX_TOLERANCE:g} pixels, got {tolerance!r}")
    return int(np.floor(t * t))


def pr_sweep(segment_preds, masks, thresholds, tolerance=2.0):
    """Tolerance-matched precision / recall counts of (segment_preds - t > 0) vs (masks > 0.5) for every threshold: int32 device tensor
    [B, 4, len(thresholds)] = (n_pred, tp_pred, tp_gt, n_gt).  A predicted pixel is a true positive when a ground-truth pixel lies within
    ``tolerance`` pixels of it (tp_pred, for the precision), a ground-truth pixel when a predicted pixel does (tp_gt, for the recall);
    distances are compared as integers, d^2 <= floor(tolerance^2), and tolerance 0 is pixel-wise matching (csrc/pr_sweep.hip)."""
    tol2 = pr_tol2(tolerance)
    L.load()
    p = _dev32(segment_preds)
    m = _dev32(masks, p)
    H, W = int(p.shape[-2]), int(p.shape[-1])
    p, m = p.reshape(-1, H, W), m.reshape(-1, H, W)
    B = p.shape[0]
    assert m.shape[0] == B, "one mask per prediction map"
    th = torch.tensor([float(t) for t in thresholds], dtype=torch.float32)          # == torch.Tensor(thresholds): fp32 roundings
    assert bool((th[1:] > th[:-1]).all()), "thresholds must ascend"
    th = th.to(p.device)
    T = th.numel()
    hist = torch.zeros(B, 3, T + 1, dtype=torch.int32, device=p.device)
    out = torch.empty(B, 4, T, dtype=torch.int32, device=p.device)
    with torch.cuda.device(p.device):
        L.call("csbsr_pr_sweep", _ptr(p), _ptr(m), _ptr(th), B, H, W, T, tol2, _ptr(hist), _ptr(out), L.stream(p.device))
    return out


# ------------------------------------------------------------------------------------------- centerlines (skeleton, clDice)
def skeleton_threshold(threshold, what="threshold"):
    """the binarisation threshold of a skeleton as a Python float: a finite float (Python or NumPy), anything else is a ValueError"""
    if not isinstance(threshold, (float, np.floating)) or not np.isfinite(threshold):
        raise ValueError(f"{what} must be a finite float, got {threshold!r}")
    return float(threshold)


def unit_threshold(threshold, what):
    """a threshold on a probability map: a float strictly inside (0, 1), anything else is a ValueError"""
    t = skeleton_threshold(threshold, what)
    if not 0.0 < t < 1.0:
        raise ValueError(f"{what} must lie strictly inside (0, 1), got {threshold!r}")
    return t


def _skeleton_passes(max_passes):
    if isinstance(max_passes, bool) or not isinstance(max_passes, (int, np.integer)) or max_passes < 0:
        raise ValueError(f"max_passes is a whole number >= 0 (0: until nothing is deleted), got {max_passes!r}")
    return int(max_passes)


def skeletonize(planes, threshold=0.5, max_passes=0):
    """Guo-Hall parallel thinning (csrc/skeleton.hip) of the planes binarised as ``planes - threshold > 0`` in fp32 (NaN -> not
    set; 0.5 on a mask is the project's ``mask > 0.5``): uint8 device tensor [N, H, W] of 0 / 1 for fp32 planes [..., H, W].  A pass is the
    first sub-iteration followed by the second; the skeleton is the plane after the first pass that deletes nothing, and ``max_passes`` =
    p > 0 gives the plane after min(p, passes to convergence) passes.  The device runs the passes in groups of up to
    csbsr_skeleton_max_passes() per launch -- the last group of a ``max_passes`` that is no multiple of it is shorter -- and the host reads
    the 4-byte count of deleted pixels back once per group, stopping at the first group that deleted nothing."""
    return _thin(planes, skeleton_threshold(threshold), _skeleton_passes(max_passes))[0]


def _thin(planes, t, p_max):
    """``skeletonize`` on checked arguments: (skeleton, launch groups, passes launched, pixels deleted)"""
    lib = L.load()
    x = _dev32(planes)
    H, W = int(x.shape[-2]), int(x.shape[-1])
    x = x.reshape(-1, H, W)
    N, dev = x.shape[0], x.device
    K = int(lib.csbsr_skeleton_max_passes())
    with torch.cuda.device(dev):
        st = L.stream(dev)
        a, b = (torch.empty(N, H, (W + 31) // 32, dtype=torch.int32, device=dev) for _ in range(2))
        deleted = torch.zeros(1, dtype=torch.int32, device=dev)          # a running total over the groups
        out = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
        L.call("csbsr_skeleton_init", _ptr(x), t, N, H, W, _ptr(a), st)
        done = total = groups = 0
        while p_max == 0 or done < p_max:
            p = K if p_max == 0 else min(K, p_max - done)
            L.call("csbsr_skeleton_passes", _ptr(a), _ptr(b), N, H, W, p, _ptr(deleted), st)
            a, b = b, a
            done, groups = done + p, groups + 1
            now = int(deleted.item())
            if now == total:
                break
            total = now
        L.call("csbsr_skeleton_finish", _ptr(a), N, H, W, _ptr(out), st)
    return out, groups, done, total


def centerline_counts(segment_preds, masks, threshold):
    """The integers of clDice: int32 device tensor [B, 4] = (|S_P|, |S_P & V_L|, |S_L|, |S_L & V_P|) with V_P = segment_preds - threshold > 0
    (fp32, NaN -> 0), V_L = masks > 0.5, and S_P, S_L their skeletons (``skeletonize``).  Scores: ``cldice_scores``, ``summarize_cldice``."""
    t = skeleton_threshold(threshold)
    L.load()
    p = _dev32(segment_preds)
    m = _dev32(masks, p)
    H, W = int(p.shape[-2]), int(p.shape[-1])
    p, m = p.reshape(-1, H, W), m.reshape(-1, H, W)
    B = p.shape[0]
    assert m.shape[0] == B, "one mask per prediction map"
    sp, sl = skeletonize(p, t), skeletonize(m, 0.5)
    out = torch.empty(B, 4, dtype=torch.int32, device=p.device)
    with torch.cuda.device(p.device):
        L.call("csbsr_centerline_counts", _ptr(sp), _ptr(p), t, _ptr(sl), _ptr(m), B, H, W, _ptr(out), L.stream(p.device))
    return out


def cldice_scores(counts):
    """(Tprec, Tsens, clDice) float64 [N] from the integer counts [N, 4] of ``centerline_counts``: Tprec = |S_P & V_L| / |S_P|, the part of the
    predicted centerline inside the ground truth; Tsens = |S_L & V_P| / |S_L|, the part of the ground-truth centerline inside the
    prediction; clDice their harmonic mean.  The conventions of ``pr_scores``: an empty S_P -> Tprec 1; an empty S_L -> Tsens 1;
    Tprec + Tsens = 0 -> clDice 0."""
    c = np.asarray(counts, dtype=np.int64)
    assert c.ndim == 2 and c.shape[1] == 4, f"counts are [N, 4], got {c.shape}"
    n_sp, sp_in, n_sl, sl_in = (c[:, i].astype(np.float64) for i in range(4))
    tp = np.where(n_sp > 0, sp_in / np.maximum(n_sp, 1.0), 1.0)
    ts = np.where(n_sl > 0, sl_in / np.maximum(n_sl, 1.0), 1.0)
    cl = np.where(tp + ts > 0, 2.0 * tp * ts / np.where(tp + ts > 0, tp + ts, 1.0), 0.0)
    return tp, ts, cl


def summarize_cldice(counts):
    """clDice, Tprec, Tsens: the means of the per-image values of ``cldice_scores``; clDice_pooled: the clDice of the counts summed over the
    images (long cracks weigh more)."""
    c = np.asarray(counts, dtype=np.int64)
    assert c.ndim == 2 and c.shape[1] == 4 and c.shape[0] >= 1
    tp, ts, cl = cldice_scores(c)
    return {"clDice": float(np.mean(cl)), "Tprec": float(np.mean(tp)), "Tsens": float(np.mean(ts)),
            "clDice_pooled": float(cldice_scores(c.sum(axis=0, keepdims=True))[2][0])}


# ------------------------------------------------------------------------------------------- connected components
CC_ACC = 5                                                   # csrc/components.hip: area_px, skeleton_px, x0, y1, x1 per root pixel
TABLE_COLUMNS = ("plane", "label", "area_px", "skeleton_px", "y0", "x0", "y1", "x1")


def component_min_px(min_px, what="min_px"):
    """the smallest component that is kept, in pixels: a whole number >= 1 (Python or NumPy, not a bool), anything else is a ValueError"""
    if isinstance(min_px, (bool, np.bool_)) or not isinstance(min_px, (int, np.integer)) or min_px < 1:
        raise ValueError(f"{what} is a whole number >= 1, got {min_px!r}")
    return int(min_px)


def _connectivity(connectivity):
    if isinstance(connectivity, (bool, np.bool_)) or not isinstance(connectivity, (int, np.integer)) or connectivity not in (4, 8):
        raise ValueError(f"connectivity is 4 or 8, got {connectivity!r}")
    return int(connectivity)


def label_components(planes, threshold=0.5, connectivity=8):
    """Connected components (csrc/components.hip) of the planes binarised as ``planes - threshold > 0`` in fp32 (NaN -> not set, the rule of
    ``skeletonize``): int32 device tensor [N, H, W] for fp32 planes [..., H, W].  A background pixel is 0, a set pixel 1 + min(y W + x) over
    its 4- or 8-connected component -- 1 + the linear index of the component's first pixel in raster order.  Planes are independent; the
    value is defined by a minimum, so two runs give the same bits."""
    t, conn = skeleton_threshold(threshold), _connectivity(connectivity)
    L.load()
    x = _dev32(planes)
    H, W = int(x.shape[-2]), int(x.shape[-1])
    x = x.reshape(-1, H, W)
    N, dev = x.shape[0], x.device
    work, labels = (torch.empty(N, H, W, dtype=torch.int32, device=dev) for _ in range(2))
    with torch.cuda.device(dev):
        L.call("csbsr_ccl_label", _ptr(x), t, N, H, W, conn, _ptr(work), _ptr(labels), L.stream(dev))
    return labels


def _labels(labels):
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.int32 and labels.dim() == 3):
        raise ValueError("labels is the int32 device tensor [N, H, W] of label_components")
    return labels.contiguous()


def _component_sums(labels, skeleton=None):
    """the accumulators of csbsr_component_sums, int32 [N, 5, H * W]: only the slots of root pixels hold values"""
    N, H, W = labels.shape
    sk = None
    if skeleton is not None:
        if not (torch.is_tensor(skeleton) and skeleton.dtype == torch.uint8 and skeleton.numel() == labels.numel()):
            raise ValueError("skeleton is a uint8 tensor with one value per label")
        sk = skeleton.to(labels.device).contiguous()
    acc = torch.empty(N, CC_ACC, H * W, dtype=torch.int32, device=labels.device)
    with torch.cuda.device(labels.device):
        L.call("csbsr_component_sums", _ptr(labels), None if sk is None else _ptr(sk), N, H, W, _ptr(acc), L.stream(labels.device))
    return acc


def _table_from_sums(labels, acc, min_px):
    """the rows of ``component_table`` from the accumulators: the roots are the pixels that carry their own index + 1, and torch.nonzero
    returns them in raster order, plane by plane -- sorted by (plane, label)"""
    N, H, W = labels.shape
    flat = labels.view(N, H * W)
    roots = torch.nonzero(flat == torch.arange(1, H * W + 1, dtype=torch.int32, device=labels.device))
    n, i = roots[:, 0], roots[:, 1]
    v = acc[n, :, i]                                         # [M, 5]
    rows = torch.stack([n, i + 1, v[:, 0], v[:, 1], torch.div(i, W, rounding_mode="floor"), v[:, 2], v[:, 3], v[:, 4]], 1).to(torch.int32)
    return rows[rows[:, 2] >= min_px] if min_px > 1 else rows


def component_table(labels, skeleton=None, min_px=1):
    """One row per component of ``label_components``' labels with at least ``min_px`` pixels: int32 device tensor [M, 8] with the columns
    (plane, label, area_px, skeleton_px, y0, x0, y1, x1), sorted by (plane, label).  The box is inclusive; ``skeleton`` (uint8 [N, H, W],
    e.g. ``skeletonize``'s) gives skeleton_px = its non-zero pixels inside the component -- the crack's length --, 0 without one."""
    k = component_min_px(min_px)
    L.load()
    labels = _labels(labels)
    return _table_from_sums(labels, _component_sums(labels, skeleton), k)


def _keep_from_sums(labels, acc, min_px, want_labels=False):
    N, H, W = labels.shape
    keep = torch.empty(N, H, W, dtype=torch.uint8, device=labels.device)
    kept = torch.empty_like(labels) if want_labels else None
    with torch.cuda.device(labels.device):
        L.call("csbsr_component_keep", _ptr(labels), _ptr(acc), N, H, W, min_px, _ptr(keep), None if kept is None else _ptr(kept),
               L.stream(labels.device))
    return keep, kept


def keep_components(labels, min_px):
    """uint8 device tensor [N, H, W]: 1 where the pixel belongs to a component of at least ``min_px`` pixels, else 0 (the speckle filter;
    min_px = 1 keeps every set pixel)."""
    k = component_min_px(min_px)
    L.load()
    labels = _labels(labels)
    return _keep_from_sums(labels, _component_sums(labels), k)[0]


# ------------------------------------------------------------------------------------------- local crack width
WIDTH_MAX_RADIUS = 128                                       # csrc/width.hip: csbsr_width_max_radius()
WIDTH_TABLE_COLUMNS = ("plane", "label", "max_d2", "y", "x")


def width_radius(max_radius, what="max_radius"):
    """the search radius of the local width, in pixels: a whole number 1 .. 128 (Python or NumPy, not a bool), anything else is a ValueError"""
    if (isinstance(max_radius, (bool, np.bool_)) or not isinstance(max_radius, (int, np.integer))
            or not 1 <= max_radius <= WIDTH_MAX_RADIUS):
        raise ValueError(f"{what} is a whole number 1 .. {WIDTH_MAX_RADIUS}, got {max_radius!r}")
    return int(max_radius)


def skeleton_width(planes, skeleton, threshold=0.5, max_radius=64):
    """The squared distance from every skeleton pixel to the nearest background pixel of its plane (csrc/width.hip): (d2, hist), int32 device
    tensors [N, H, W] and [N, r^2 + 2] for fp32 planes [..., H, W] and a uint8 skeleton of the same shape (``skeletonize``'s, or any subset
    of it).  The region is ``planes - threshold > 0`` in fp32 (NaN -> not set), the background the other pixels of the SAME plane: the image
    border, the next plane and the padding of a packed row are no background.  d2 = min(r^2 + 1, the exact squared distance) at a skeleton
    pixel -- r^2 + 1 means wider than the search radius r = ``max_radius``: saturated --, 0 elsewhere and at a skeleton pixel outside the
    region.  hist[n][v] counts the skeleton pixels of plane n with d2 == v.  The local width is ``width_from_d2``."""
    t, r = skeleton_threshold(threshold), width_radius(max_radius)
    L.load()
    x = _dev32(planes)
    if not (torch.is_tensor(skeleton) and skeleton.dtype == torch.uint8):
        raise ValueError("skeleton is a uint8 tensor of the planes' shape")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    x = x.reshape(-1, H, W)
    if skeleton.dim() < 2 or tuple(skeleton.shape[-2:]) != (H, W) or skeleton.numel() != x.numel():      # [N, H, W] or the planes' own shape
        raise ValueError(f"the skeleton is {tuple(skeleton.shape)}, the planes are {tuple(planes.shape)}")
    N, dev = x.shape[0], x.device
    sk = skeleton.to(dev).contiguous()
    d2 = torch.empty(N, H, W, dtype=torch.int32, device=dev)
    hist = torch.empty(N, r * r + 2, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("csbsr_skeleton_width", _ptr(x), t, _ptr(sk), N, H, W, r, _ptr(d2), _ptr(hist), L.stream(dev))
    return d2, hist


def _component_width(labels, d2):
    """the accumulators of csbsr_component_width, int32 [N, 2, H * W]: only the slots of root pixels hold values"""
    N, H, W = labels.shape
    if not (torch.is_tensor(d2) and d2.dtype == torch.int32 and tuple(d2.shape) == (N, H, W)):
        raise ValueError("d2 is the int32 tensor [N, H, W] of skeleton_width, one value per label")
    d2 = d2.to(labels.device).contiguous()
    wacc = torch.empty(N, 2, H * W, dtype=torch.int32, device=labels.device)
    with torch.cuda.device(labels.device):
        L.call("csbsr_component_width", _ptr(labels), _ptr(d2), N, H, W, _ptr(wacc), L.stream(labels.device))
    return wacc


def _width_columns(table, wacc, W):
    """(max_d2, y, x) int32 [M, 3] for the rows of a component table (plane, label, ...): y = x = -1 where max_d2 is 0"""
    n, i = table[:, 0].long(), table[:, 1].long() - 1
    m, at = wacc[n, 0, i], wacc[n, 1, i]
    y = torch.where(at >= 0, torch.div(at, W, rounding_mode="floor"), at)
    return torch.stack([m, y, torch.where(at >= 0, at - y * W, at)], 1).to(torch.int32)


def component_width_table(labels, d2, min_px=1):
    """The widest point of every component: int32 device tensor [M, 5] = (plane, label, max_d2, y, x) with exactly the rows of
    ``component_table(labels, None, min_px)``, in that order.  max_d2 is the largest ``d2`` (``skeleton_width``'s) over the component's pixels,
    (y, x) the first pixel in raster order that attains it; a component without a pixel of d2 > 0 has (0, -1, -1)."""
    rows = component_table(labels, None, min_px)
    labels = _labels(labels)
    return torch.cat([rows[:, :2], _width_columns(rows, _component_width(labels, d2), labels.shape[2])], 1)


def _host_ints(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def width_from_d2(d2):
    """the local width in pixels, fp64 on the host: 2 sqrt(d2) - 1, and 0.0 where d2 = 0 (ints, NumPy arrays or tensors; a Python float for a
    scalar).  A straight bar of odd width w gives exactly w on its centerline; an even width w gives w - 1, because the centerline lies on one
    of the two middle rows -- this one-pixel bias is left as it is."""
    d = _host_ints(d2).astype(np.float64)
    w = np.where(d > 0, 2.0 * np.sqrt(d) - 1.0, 0.0)
    return float(w) if w.ndim == 0 else w


def _hist_row(hist_row):
    h = _host_ints(hist_row).astype(np.int64)
    if h.ndim != 1 or h.size < 3:
        raise ValueError(f"a width histogram is one plane's row of r^2 + 2 counts, got shape {h.shape}")
    return h


def summarize_width_hist(hist_row, max_radius):
    """The width figures of one plane from its histogram (``skeleton_width``'s hist[n]), fp64 on the host: centerline_px (the bins >= 1),
    outside_px (bin 0), saturated_px (the last bin), and over the centerline pixels' local widths (``width_from_d2``) centerline_width_px
    (their mean), median_width_px (the element of zero-based rank (n - 1) // 2 of the sorted d2), p95_width_px (rank ceil(0.95 n) - 1) and
    max_width_px.  Saturated pixels take part with r^2 + 1: with saturated_px > 0 the figures are lower bounds.  n = 0: every width 0.0."""
    r = width_radius(max_radius)
    h = _hist_row(hist_row)
    if h.size != r * r + 2:
        raise ValueError(f"the histogram of radius {r} has {r * r + 2} bins, got {h.size}")
    c = h[1:]
    n = int(c.sum())
    out = {"centerline_px": n, "outside_px": int(h[0]), "saturated_px": int(h[-1])}
    if n == 0:
        out.update(centerline_width_px=0.0, median_width_px=0.0, p95_width_px=0.0, max_width_px=0.0)
        return out
    w = width_from_d2(np.arange(1, h.size))
    cum = np.cumsum(c)
    at = lambda rank: float(w[int(np.searchsorted(cum, rank + 1))])                 # the first bin whose cumulative count exceeds the rank
    out.update(centerline_width_px=float(np.dot(c.astype(np.float64), w) / n), median_width_px=at((n - 1) // 2),
               p95_width_px=at(-(-95 * n // 100) - 1), max_width_px=float(w[int(np.nonzero(c)[0][-1])]))
    return out


def centerline_px_at_least(hist_row, width_px):
    """the centerline pixels whose local width is >= ``width_px``, from one plane's histogram: the length of crack wider than a limit
    (saturated pixels count with the width of r^2 + 1; bin 0 never counts)"""
    h = _hist_row(hist_row)
    w = width_from_d2(np.arange(1, h.size))
    return int(h[1:][w >= float(width_px)].sum())


# ------------------------------------------------------------------------------------------- crack topology
TOPO_COUNTS = 10                                             # csrc/topology.hip: the counters per plane
TOPO_ACC = 9                                                 # and the accumulators per root pixel
TOPOLOGY_COLUMNS = ("V", "isolated", "end", "path", "junction_px", "h", "v", "d_se", "d_sw", "q4")
TOPOLOGY_TABLE_COLUMNS = ("plane", "label", "end", "junction_px", "h", "v", "d_se", "d_sw", "q4", "isolated", "junctions")
TOPO_ISOLATED, TOPO_END, TOPO_PATH, TOPO_JUNCTION = 1, 2, 3, 4        # bits 0-2 of a topo byte
TOPO_QUAD, TOPO_E, TOPO_S, TOPO_SE, TOPO_SW = 8, 16, 32, 64, 128      # and its flags


def skeleton_topology(skeleton):
    """Node class, owned links and full quads of every pixel of binary planes (csrc/topology.hip): (topo, counts), device tensors
    uint8 [N, H, W] and int32 [N, 10], for a uint8 tensor [..., H, W] that is set where it is non-zero (``skeletonize``'s, or any other).
    topo: bits 0-2 the class -- 0 clear, 1 isolated, 2 end, 3 path, 4 junction --, bit 3 the pixel owns a full quad, bits 4 .. 7 it owns an
    E, S, SE, SW link.  counts: ``TOPOLOGY_COLUMNS`` per plane.  Planes are independent and nothing outside a plane is set."""
    if not (torch.is_tensor(skeleton) and skeleton.dtype == torch.uint8 and skeleton.dim() >= 2):
        raise ValueError("skeleton is a uint8 tensor [..., H, W]")
    L.load()
    dev = skeleton.device if skeleton.is_cuda else torch.device("cuda:0")
    H, W = int(skeleton.shape[-2]), int(skeleton.shape[-1])
    sk = skeleton.to(dev).reshape(-1, H, W).contiguous()
    N = sk.shape[0]
    topo = torch.empty(N, H, W, dtype=torch.uint8, device=dev)
    counts = torch.empty(N, TOPO_COUNTS, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("csbsr_skeleton_topology", _ptr(sk), N, H, W, _ptr(topo), _ptr(counts), L.stream(dev))
    return topo, counts


def _junction_labels(topo):
    """the 8-connected clusters of the junction pixels of ``skeleton_topology``'s topo, labelled by ``label_components``"""
    return label_components(((topo & 7) == TOPO_JUNCTION).to(torch.float32), 0.5)


def _count_roots(labels):
    """the components per plane, int64 [N]: the pixels that carry their own linear index + 1"""
    N, H, W = labels.shape
    return (labels.view(N, H * W) == torch.arange(1, H * W + 1, dtype=torch.int32, device=labels.device)).sum(1)


def _component_topology(labels, topo, jlabels=None):
    """the accumulators of csbsr_component_topology, int32 [N, 9, H * W]: only the slots of root pixels hold values"""
    N, H, W = labels.shape
    if not (torch.is_tensor(topo) and topo.dtype == torch.uint8 and tuple(topo.shape) == (N, H, W)):
        raise ValueError("topo is the uint8 tensor [N, H, W] of skeleton_topology, one value per label")
    topo = topo.to(labels.device).contiguous()
    tacc = torch.empty(N, TOPO_ACC, H * W, dtype=torch.int32, device=labels.device)
    with torch.cuda.device(labels.device):
        L.call("csbsr_component_topology", _ptr(labels), _ptr(topo), None if jlabels is None else _ptr(jlabels), N, H, W, _ptr(tacc),
               L.stream(labels.device))
    return tacc


def _topology_columns(table, tacc):
    """the nine sums, int32 [M, 9], for the rows of a component table (plane, label, ...)"""
    return tacc[table[:, 0].long(), :, table[:, 1].long() - 1]


def component_topology_table(labels, topo, min_px=1):
    """The topology sums of every component: int32 device tensor [M, 11] = ``TOPOLOGY_TABLE_COLUMNS`` with exactly the rows of
    ``component_table(labels, None, min_px)``, in that order.  The sums run over the component's pixels of ``topo`` (``skeleton_topology``'s);
    junctions counts the 8-connected clusters of junction pixels by their first pixel in raster order."""
    rows = component_table(labels, None, min_px)
    labels = _labels(labels)
    if not (torch.is_tensor(topo) and topo.dtype == torch.uint8 and tuple(topo.shape) == tuple(labels.shape)):
        raise ValueError("topo is the uint8 tensor [N, H, W] of skeleton_topology, one value per label")
    topo = topo.to(labels.device).contiguous()
    return torch.cat([rows[:, :2], _topology_columns(rows, _component_topology(labels, topo, _junction_labels(topo)))], 1)


_SQRT2 = float(np.sqrt(2.0))


def geodesic_length(h, v, d_se, d_sw):
    """the chain-code length between pixel centres, fp64 on the host: h + v + sqrt(2) (d_se + d_sw) (ints, NumPy arrays or tensors; a Python
    float for scalars).  A straight run of n pixels gives n - 1, a 45-degree run sqrt(2) (n - 1); a straight line at another angle reads long
    by up to 8.24 % (at 22.5 degrees) -- this bias is left as it is, like the even-width bias of ``width_from_d2``."""
    h, v, a, b = (_host_ints(t).astype(np.float64) for t in (h, v, d_se, d_sw))
    n = h + v + _SQRT2 * (a + b)
    return float(n) if n.ndim == 0 else n


def orientation_shares(h, v, d_se, d_sw):
    """the shares of the geodesic length that run horizontally, vertically and along the two diagonals: a 4-tuple of Python floats that sums
    to 1, all zeros for a length of 0"""
    parts = (float(h), float(v), _SQRT2 * float(d_se), _SQRT2 * float(d_sw))
    n = geodesic_length(h, v, d_se, d_sw)
    return tuple(p / n for p in parts) if n > 0 else (0.0, 0.0, 0.0, 0.0)


def euler_number(V, links, q4):
    """chi = V - (h + v + d_se + d_sw) + q4 of the cell complex of set pixels, owned links and full quads: components minus enclosed cells"""
    return int(V) - sum(int(k) for k in links) + int(q4)


def mean_width_geodesic(crack_px, length):
    """crack_px / length in fp64, 0.0 for a length of 0"""
    return float(crack_px) / float(length) if length else 0.0


def summarize_topology(counts_row, n_components, n_junctions):
    """The topology figures of one plane from its row of ``skeleton_topology``'s counts, the number of 8-connected components of the plane and
    the number of junction clusters: a dict of skeleton_px, endpoints, junctions, junction_px, isolated_px, path_px, links = (h, v, d_se,
    d_sw), quads, euler, components, loops = components - euler (the enclosed cells), length_geodesic_px and orientation."""
    c = _host_ints(counts_row).astype(np.int64)
    if c.shape != (TOPO_COUNTS,):
        raise ValueError(f"a row of topology counts has {TOPO_COUNTS} integers, got shape {c.shape}")
    V, iso, end, path, jpx, h, v, dse, dsw, q4 = (int(k) for k in c)
    links = (h, v, dse, dsw)
    chi = euler_number(V, links, q4)
    return {"skeleton_px": V, "endpoints": end, "junctions": int(n_junctions), "junction_px": jpx, "isolated_px": iso, "path_px": path,
            "links": links, "quads": q4, "euler": chi, "components": int(n_components), "loops": int(n_components) - chi,
            "length_geodesic_px": geodesic_length(*links), "orientation": orientation_shares(*links)}


# ------------------------------------------------------------------------------------------- spur pruning
PRUNE_MAX_SPUR = 64                                          # csrc/prune.hip: csbsr_prune_max_spur()


def spur_length(spur_px, what="spur_px"):
    """the longest side branch that is pruned, in pixels: a whole number 1 .. 64 (Python or NumPy, not a bool), anything else is a ValueError"""
    if isinstance(spur_px, (bool, np.bool_)) or not isinstance(spur_px, (int, np.integer)) or not 1 <= spur_px <= PRUNE_MAX_SPUR:
        raise ValueError(f"{what} is a whole number 1 .. {PRUNE_MAX_SPUR}, got {spur_px!r}")
    return int(spur_px)


def prune_spurs(skeleton, spur_px, return_time=False):
    """The planes without their side branches of up to ``spur_px`` pixels (csrc/prune.hip): (pruned, removed), device tensors
    uint8 [N, H, W] of 0 / 1 and int32 [N], for a uint8 tensor [..., H, W] that is set where it is non-zero (``skeletonize``'s, or any other);
    removed = the set pixels of a plane minus those of its result.  Tips (end pixels with at most 3 neighbours) are peeled ``spur_px``
    times, each step recording its number T at the pixels it deletes, and grown back in reverse order from the tips that are left: what was
    peeled from a surviving end returns exactly, a branch that was peeled down to a junction does not, and of the arms of a fork at a
    crack's end only the longest -- or all the longest -- return.  ``return_time`` = True adds T, uint8 [N, H, W], as a third result.  Planes
    are independent, nothing outside a plane is set, and nothing is read by the host."""
    L_px = spur_length(spur_px)
    if not (torch.is_tensor(skeleton) and skeleton.dtype == torch.uint8 and skeleton.dim() >= 2):
        raise ValueError("skeleton is a uint8 tensor [..., H, W]")
    lib = L.load()
    dev = skeleton.device if skeleton.is_cuda else torch.device("cuda:0")
    H, W = int(skeleton.shape[-2]), int(skeleton.shape[-1])
    sk = skeleton.to(dev).reshape(-1, H, W).contiguous()
    N = sk.shape[0]
    need = int(lib.csbsr_prune_work_bytes(N, H, W))
    if need <= 0:
        raise L.CsbsrHipError(f"prune_spurs: {N} planes of {H} x {W} are outside what csbsr_skeleton_prune takes")
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    out, time = (torch.empty(N, H, W, dtype=torch.uint8, device=dev) for _ in range(2))
    removed = torch.empty(N, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.call("csbsr_skeleton_prune", _ptr(sk), N, H, W, L_px, _ptr(work), _ptr(time), _ptr(out), _ptr(removed), L.stream(dev))
    return (out, removed, time) if return_time else (out, removed)


# ------------------------------------------------------------------------------------------- crack branches
BRANCH_ACC = 12                                              # csrc/branches.hip: the accumulators per root pixel, and two more with a d2 map
BRANCH_COLUMNS = ("plane", "label", "crack", "px", "end", "isolated", "attach", "h", "v", "d_se", "d_sw", "node_a", "node_b", "y0", "x0", "y1",
                  "x1")
BRANCH_WIDTH_COLUMNS = ("max_d2", "min_d2")                  # behind BRANCH_COLUMNS when ``branch_table`` is given a d2 map
BRANCH_KINDS = ("isolated", "free", "ring", "terminal", "self_loop", "link")


def _topo(topo):
    if not (torch.is_tensor(topo) and topo.dtype == torch.uint8 and topo.dim() == 3):
        raise ValueError("topo is the uint8 tensor [N, H, W] of skeleton_topology")
    return (topo if topo.is_cuda else topo.to("cuda:0")).contiguous()


def label_branches(topo):
    """The branches of ``skeleton_topology``'s topo (csrc/branches.hip): int32 device tensor [N, H, W].  A branch pixel is a set
    pixel that is no junction (class 1, 2 or 3), a branch a connected component of the branch pixels under the owned links between two of
    them -- the centerline segments between junctions; an isolated pixel is a branch of one pixel.  The value is 0 at clear and at junction
    pixels, else 1 + min(y W + x) over the pixel's branch: defined by a minimum, so two runs give the same bits.  Planes are independent."""
    topo = _topo(topo)
    L.load()
    N, H, W = topo.shape
    work, blabels = (torch.empty(N, H, W, dtype=torch.int32, device=topo.device) for _ in range(2))
    with torch.cuda.device(topo.device):
        L.call("csbsr_branch_label", _ptr(topo), N, H, W, _ptr(work), _ptr(blabels), L.stream(topo.device))
    return blabels


def _plane_like(t, like, what):
    if not (torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == tuple(like.shape)):
        raise ValueError(f"{what} is an int32 tensor {tuple(like.shape)}, one value per branch label")
    return t.to(like.device).contiguous()


def _branch_sums(blabels, topo, jlabels=None, d2=None):
    """the accumulators of csbsr_branch_sums, int32 [N, 12 or 14, H * W]: only the slots of root pixels hold values"""
    N, H, W = blabels.shape
    bacc = torch.empty(N, BRANCH_ACC + (0 if d2 is None else 2), H * W, dtype=torch.int32, device=blabels.device)
    with torch.cuda.device(blabels.device):
        L.call("csbsr_branch_sums", _ptr(blabels), _ptr(topo), None if jlabels is None else _ptr(jlabels), None if d2 is None else _ptr(d2),
               N, H, W, _ptr(bacc), L.stream(blabels.device))
    return bacc


def branch_table(blabels, topo, jlabels=None, labels=None, d2=None):
    """One row per branch of ``label_branches``' labels: int32 device tensor [M, 17] = ``BRANCH_COLUMNS``, in raster order of the branch's
    first pixel, plane by plane -- sorted by (plane, label).  px: the branch's pixels; end: its end pixels (class 2); isolated: 1 for a
    class-1 pixel; h, v, d_se, d_sw: its links of each kind, those between two of its pixels and those that attach it to a junction pixel
    (whichever end owns the link), so that ``geodesic_length`` runs from junction pixel centre to junction pixel centre; attach: its attach
    links; node_a, node_b: the smallest and largest value of ``jlabels`` (the junction clusters, ``label_components`` of the class-4 mask)
    among the junction pixels it attaches to -- 0 and 0 without an attach link or without ``jlabels``; a branch that touches three or more
    clusters reports only these two, and its attach exceeds 2 --; (y0, x0, y1, x1): the inclusive box.  crack is ``labels`` (e.g. the
    component labels of ``label_components``) at the branch's first pixel, 0 without.  With ``d2`` (``skeleton_width``'s) two more columns,
    ``BRANCH_WIDTH_COLUMNS``: the largest d2 and the smallest d2 > 0 over the branch's pixels (0 if none)."""
    if not (torch.is_tensor(blabels) and blabels.is_cuda and blabels.dtype == torch.int32 and blabels.dim() == 3):
        raise ValueError("blabels is the int32 device tensor [N, H, W] of label_branches")
    L.load()
    blabels = blabels.contiguous()
    N, H, W = blabels.shape
    if not (torch.is_tensor(topo) and topo.dtype == torch.uint8 and tuple(topo.shape) == (N, H, W)):
        raise ValueError("topo is the uint8 tensor [N, H, W] of skeleton_topology, one value per branch label")
    topo = topo.to(blabels.device).contiguous()
    jlabels, labels, d2 = (None if t is None else _plane_like(t, blabels, what) for t, what in ((jlabels, "jlabels"), (labels, "labels"), (d2, "d2")))
    bacc = _branch_sums(blabels, topo, jlabels, d2)
    flat = blabels.view(N, H * W)
    roots = torch.nonzero(flat == torch.arange(1, H * W + 1, dtype=torch.int32, device=blabels.device))
    n, i = roots[:, 0], roots[:, 1]
    v = bacc[n, :, i].to(torch.int64)                        # [M, 12 or 14]
    crack = labels.view(N, H * W)[n, i].to(torch.int64) if labels is not None else torch.zeros_like(i)
    isolated = ((topo.view(N, H * W)[n, i] & 7) == TOPO_ISOLATED).to(torch.int64)
    cols = [n, i + 1, crack, v[:, 0], v[:, 1], isolated] + [v[:, k] for k in range(2, 9)] + [torch.div(i, W, rounding_mode="floor"), v[:, 9], v[:, 10],
                                                                                            v[:, 11]]
    return torch.stack(cols + ([v[:, 12], v[:, 13]] if d2 is not None else []), 1).to(torch.int32)


def branch_kind(end, attach, node_a, node_b, isolated):
    """what a branch is, from its row of ``branch_table``: 'isolated' (a class-1 pixel), 'free' (no attach link and two ends: a crack without
    a junction), 'ring' (no attach link and no end: a closed loop without a junction), 'terminal' (an end and an attach link: a dead end),
    'self_loop' (no end, attached, and node_a == node_b: it leaves and re-enters one junction cluster) or 'link' (the rest: it joins two
    junction clusters).  The node columns need the table's ``jlabels``."""
    end, attach = int(end), int(attach)
    if int(isolated):
        return "isolated"
    if attach == 0 and end == 2:
        return "free"
    if attach == 0 and end == 0:
        return "ring"
    if end >= 1 and attach >= 1:
        return "terminal"
    if end == 0 and attach >= 1 and int(node_a) == int(node_b):
        return "self_loop"
    return "link"


def _branch_rows(rows):
    r = _host_ints(rows).astype(np.int64)
    if r.ndim != 2 or r.shape[1] not in (len(BRANCH_COLUMNS), len(BRANCH_COLUMNS) + len(BRANCH_WIDTH_COLUMNS)):
        raise ValueError(f"branch rows are [M, {len(BRANCH_COLUMNS)}] or [M, {len(BRANCH_COLUMNS) + len(BRANCH_WIDTH_COLUMNS)}] integers "
                         f"(branch_table), got shape {r.shape}")
    return r


def branch_kinds(rows):
    """the kind (``branch_kind``) of every row of ``branch_table``, a list of strings: the truth table on whole columns"""
    r = _branch_rows(rows)
    c = {k: j for j, k in enumerate(BRANCH_COLUMNS)}
    end, attach, same = r[:, c["end"]], r[:, c["attach"]], r[:, c["node_a"]] == r[:, c["node_b"]]
    k = np.select([r[:, c["isolated"]] != 0, (attach == 0) & (end == 2), (attach == 0) & (end == 0), (end >= 1) & (attach >= 1),
                   (end == 0) & (attach >= 1) & same], [0, 1, 2, 3, 4], 5)
    return [BRANCH_KINDS[j] for j in k.tolist()]


def summarize_branches(rows):
    """The branch figures of one plane (or of any set of rows of ``branch_table``), fp64 on the host: n_branches, branch_kinds (a dict over
    ``BRANCH_KINDS`` of counts), and over the geodesic lengths (``geodesic_length`` of h, v, d_se, d_sw) of the branches that are not
    isolated: longest_branch_px, median_branch_px (the element of zero-based rank (n - 1) // 2 of the sorted lengths) and total_branch_px.
    No such branch: the three lengths are 0.0."""
    r = _branch_rows(rows)
    c = {k: j for j, k in enumerate(BRANCH_COLUMNS)}
    kinds = branch_kinds(r)
    out = {"n_branches": int(r.shape[0]), "branch_kinds": {k: kinds.count(k) for k in BRANCH_KINDS}}
    length = np.sort(np.asarray(geodesic_length(r[:, c["h"]], r[:, c["v"]], r[:, c["d_se"]], r[:, c["d_sw"]]), np.float64)[r[:, c["isolated"]] == 0])
    n = int(length.size)
    out.update(longest_branch_px=float(length[-1]) if n else 0.0, median_branch_px=float(length[(n - 1) // 2]) if n else 0.0,
               total_branch_px=float(length.sum()) if n else 0.0)
    return out


# ------------------------------------------------------------------------------------------- crack polylines
ORDER_COLUMNS = ("y", "x", "diag", "d2")                     # a row of ``branch_polylines``' points
PL_MAX_P = 1 << 28                                           # csrc/polylines.hip: the branch pixels one call orders


def order_branches(blabels, topo, return_rounds=False):
    """The position of every branch pixel along its branch (csrc/polylines.hip): (rank, diag), int32 device tensors [N, H, W],
    for ``label_branches``' labels and ``skeleton_topology``'s topo.  The degree of a branch pixel is the number of its inner links; a
    branch is a chain when no pixel of it has a degree above 2.  A chain with terminals (degree <= 1) starts at the terminal with the
    smaller linear index y W + x; a chain without one (a cycle) starts at its first pixel in raster order and is walked from there first to
    the start's neighbour with the smaller linear index.  rank = the inner links walked from the start (0 .. px - 1), diag = the SE / SW
    links among them; both are -1 at clear pixels, at junction pixels and at every pixel of a branch that is no chain (a branch through a
    full 2 x 2 quad).  The device ranks the compact list of the call's P branch pixels by pointer jumping in R = ceil(log2(P)) launches,
    whatever the branches' lengths; the host reads P (8 bytes) once to size the list.  ``return_rounds`` = True adds R as a third result."""
    if not (torch.is_tensor(blabels) and blabels.is_cuda and blabels.dtype == torch.int32 and blabels.dim() == 3):
        raise ValueError("blabels is the int32 device tensor [N, H, W] of label_branches")
    lib = L.load()
    blabels = blabels.contiguous()
    N, H, W = blabels.shape
    dev = blabels.device
    if not (torch.is_tensor(topo) and topo.dtype == torch.uint8 and tuple(topo.shape) == (N, H, W)):
        raise ValueError("topo is the uint8 tensor [N, H, W] of skeleton_topology, one value per branch label")
    topo = topo.to(dev).contiguous()
    rank, diag = (torch.empty(N, H, W, dtype=torch.int32, device=dev) for _ in range(2))
    count = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = L.stream(dev)
        L.call("csbsr_branch_count", _ptr(topo), N, H, W, _ptr(count), st)
        P = int(count.item())                                # the one read: it sizes the list and the rounds
        need = int(lib.csbsr_branch_order_work_bytes(P)) if P <= PL_MAX_P else 0
        if need <= 0:
            raise L.CsbsrHipError(f"order_branches: {P} branch pixels are more than one call orders ({PL_MAX_P})")
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        L.call("csbsr_branch_order", _ptr(topo), _ptr(blabels), N, H, W, P, _ptr(work), _ptr(rank), _ptr(diag), st)
    return (rank, diag, int(lib.csbsr_branch_order_rounds(P))) if return_rounds else (rank, diag)


def branch_polylines(blabels, rank, diag, d2=None):
    """The ordered points of every branch: (chain, offsets, points) -- bool [M], int64 [M + 1] and int32 [P_chain, 4] device tensors -- for
    ``label_branches``' labels and ``order_branches``' rank and diag.  The M rows are those of ``branch_table``, in its order; row j's
    points are points[offsets[j]:offsets[j + 1]], ``ORDER_COLUMNS`` = (y, x, diag, d2) per pixel from the branch's start to its stop, d2
    from ``d2`` (``skeleton_width``'s) or 0.  chain[j] is False for a branch that ``order_branches`` left unordered; its span is empty.  No
    sort: the device writes every pixel to row offsets[j] + rank."""
    if not (torch.is_tensor(blabels) and blabels.is_cuda and blabels.dtype == torch.int32 and blabels.dim() == 3):
        raise ValueError("blabels is the int32 device tensor [N, H, W] of label_branches")
    L.load()
    blabels = blabels.contiguous()
    N, H, W = blabels.shape
    dev = blabels.device
    rank, diag = _plane_like(rank, blabels, "rank"), _plane_like(diag, blabels, "diag")
    d2 = None if d2 is None else _plane_like(d2, blabels, "d2")
    hw = H * W
    flat, rk = blabels.view(N, hw), rank.view(-1)
    roots = torch.nonzero(flat == torch.arange(1, hw + 1, dtype=torch.int32, device=dev))
    root_g = roots[:, 0] * hw + roots[:, 1]                  # ascending: the order of branch_table
    chain = rk[root_g] >= 0
    at = torch.nonzero(rk >= 0).view(-1)                     # the ordered pixels
    if at.numel() > 2 ** 31 - 1:
        raise ValueError(f"{at.numel()} ordered pixels do not fit the int32 rows of one table")
    key = torch.div(at, hw, rounding_mode="floor") * hw + blabels.view(-1)[at].to(torch.int64) - 1
    px = torch.bincount(torch.searchsorted(root_g, key), minlength=root_g.numel())[:root_g.numel()]
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(px * chain, 0)])
    first = torch.empty(N * hw, dtype=torch.int32, device=dev)       # only the slots of root pixels hold values
    first[root_g] = offsets[:-1].to(torch.int32)
    points = torch.empty(at.numel(), 4, dtype=torch.int32, device=dev)
    if at.numel() == 0:
        return chain, offsets, points
    with torch.cuda.device(dev):
        L.call("csbsr_branch_scatter", _ptr(blabels), _ptr(rank), _ptr(diag), None if d2 is None else _ptr(d2), _ptr(first), N, H, W,
               int(at.numel()), _ptr(points), L.stream(dev))
    return chain, offsets, points


def arc_position(rank, diag):
    """the chain-code distance from the branch's start, fp64 on the host: (rank - diag) + sqrt(2) diag (ints, NumPy arrays or tensors; a
    Python float for scalars).  It shares the bias of ``geodesic_length``."""
    r, d = _host_ints(rank).astype(np.float64), _host_ints(diag).astype(np.float64)
    s = (r - d) + _SQRT2 * d
    return float(s) if s.ndim == 0 else s


def _diag_along(points):
    """int64 [px]: the diagonal steps up to each point of one branch's (y, x) rows"""
    p = _host_ints(points).astype(np.int64)
    if p.ndim != 2 or p.shape[1] < 2:
        raise ValueError(f"points are [px, 2 or more] integers, y and x first, got shape {p.shape}")
    step = np.diff(p[:, :2], axis=0)
    return np.concatenate([np.zeros(min(1, p.shape[0]), np.int64), np.cumsum((step[:, 0] != 0) & (step[:, 1] != 0))])


def polyline_stats(points, cycle=False):
    """The figures of one branch's ordered points [px, 2 or more] (y and x first: a span of ``branch_polylines``' points), fp64 on the host:
    start and stop, (y, x) tuples; arc_px, the chain-code length of the px - 1 inner links between them (``arc_position`` of the last
    point); chord_px, the distance from start to stop; tortuosity = arc_px / chord_px, None when the chord is 0 or the branch is a cycle
    (``cycle`` = True: the points do not tell -- the two ends of a path can be neighbours without a link); direction_deg, atan2(dy, dx) of
    stop - start folded to [0, 180), None with a zero chord.  No point: start and stop are None, the lengths 0.0."""
    p = _host_ints(points).astype(np.int64)
    if p.size == 0:
        return {"start": None, "stop": None, "arc_px": 0.0, "chord_px": 0.0, "tortuosity": None, "direction_deg": None}
    nd = int(_diag_along(p)[-1])
    arc = arc_position(p.shape[0] - 1, nd)
    dy, dx = int(p[-1, 0] - p[0, 0]), int(p[-1, 1] - p[0, 1])
    chord = math.sqrt(float(dy * dy + dx * dx))
    return {"start": (int(p[0, 0]), int(p[0, 1])), "stop": (int(p[-1, 0]), int(p[-1, 1])), "arc_px": arc, "chord_px": chord,
            "tortuosity": None if chord == 0 or cycle else arc / chord,
            "direction_deg": None if chord == 0 else math.degrees(math.atan2(dy, dx)) % 180.0}


# ------------------------------------------------------------------------------------------- simplified polylines
SIMPLIFY_MAX_PX = 16.0                                       # csrc/simplify.hip: SP_MAX_TOL_Q quarter pixels
SIMPLIFY_ROUTE_LIMITS = (64, 2048)                           # csrc/simplify.hip: SP_WAVE_MAX, SP_LDS_MAX -- the longest span of a wave, of LDS


def simplify_tolerance(px, what="tolerance_px"):
    """the tolerance in quarter pixels: ``px`` is an int or a float (Python or NumPy, not a bool) that is an exact multiple of 0.25 in
    [0, 16]; anything else is a ValueError"""
    ok = not isinstance(px, (bool, np.bool_)) and isinstance(px, (int, float, np.integer, np.floating))
    if ok:
        q = float(px) * 4.0                                  # exact: a power of two
        ok = math.isfinite(q) and q == math.floor(q) and 0.0 <= q <= 4.0 * SIMPLIFY_MAX_PX
    if not ok:
        raise ValueError(f"{what} is a multiple of 0.25 in [0, {SIMPLIFY_MAX_PX:g}], got {px!r}")
    return int(q)


def simplify_polylines(offsets, points, tolerance_px):
    """Douglas-Peucker on every span of ``branch_polylines``' table (csrc/simplify.hip): (keep, voffsets, vindex) -- uint8 [P],
    int64 [M + 1] and int32 [V] device tensors -- for offsets int64 [M + 1] and points int32 [P, 4] (only y and x are read) on the device.
    keep is 1 at the rows that stay; vindex holds those rows ascending, so the vertices are points[vindex], and span j's are
    vindex[voffsets[j]:voffsets[j + 1]].  The first and the last row of a span always stay; an inner row stays iff it is the farthest from
    the segment between its kept neighbours (the smallest row among equals) and farther than ``tolerance_px`` (``simplify_tolerance``),
    compared in integers.  A closed chain is the open polyline from its first to its last row.  Nothing is read by the host."""
    tol_q = simplify_tolerance(tolerance_px)
    if not (torch.is_tensor(offsets) and offsets.is_cuda and offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.numel() >= 1):
        raise ValueError("offsets is the int64 device tensor [M + 1] of branch_polylines")
    if not (torch.is_tensor(points) and points.is_cuda and points.dtype == torch.int32 and points.dim() == 2 and points.shape[1] == 4
            and points.device == offsets.device):
        raise ValueError("points is the int32 device tensor [P, 4] of branch_polylines, on the device of offsets")
    lib = L.load()
    dev = offsets.device
    offsets, points = offsets.contiguous(), points.contiguous()
    M, P = offsets.numel() - 1, points.shape[0]
    if M == 0 or P == 0:
        return torch.zeros(P, dtype=torch.uint8, device=dev), torch.zeros(M + 1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    need = int(lib.csbsr_polyline_simplify_work_bytes(M, P)) if M <= PL_MAX_P and P <= PL_MAX_P else 0
    if need <= 0:
        raise L.CsbsrHipError(f"simplify_polylines: {M} spans over {P} rows are more than one call takes ({PL_MAX_P})")
    keep = torch.empty(P, dtype=torch.uint8, device=dev)     # the entry writes every row
    vcount = torch.empty(M, dtype=torch.int32, device=dev)
    work = torch.empty(need, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.call("csbsr_polyline_simplify", _ptr(offsets), _ptr(points), M, P, tol_q, _ptr(work), _ptr(keep), _ptr(vcount), L.stream(dev))
    voffsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(vcount, 0, dtype=torch.int64)])
    return keep, voffsets, torch.nonzero(keep).view(-1).to(torch.int32)


def polyline_length(yx, closed=False):
    """the Euclidean length of the polyline through the vertices ``yx`` [v, 2 or more] (y and x first), fp64 on the host: the sum of its
    segments' lengths, with ``closed`` also the segment from the last vertex back to the first; 0.0 for fewer than two vertices"""
    p = _host_ints(yx).astype(np.float64)
    if p.ndim != 2 or p.shape[1] < 2:
        raise ValueError(f"yx is [v, 2 or more], y and x first, got shape {p.shape}")
    p = p[:, :2]
    if p.shape[0] < 2:
        return 0.0
    if closed:
        p = np.concatenate([p, p[:1]])
    d = np.diff(p, axis=0)
    return float(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).sum())


# ------------------------------------------------------------------------------------------- crack gap bridging
GAP_MAX_RADIUS = 64                                          # csrc/gaps.hip: csbsr_gap_max_radius()
GAP_COLUMNS = ("plane", "p", "q", "d2", "label_p", "label_q", "class_q", "mutual")
GAP_TO = ("any", "end")


def gap_radius(G, what="max_gap"):
    """the largest gap that is bridged, in pixels: a whole number 2 .. 64 (Python or NumPy, not a bool), anything else is a ValueError.  Two
    different 8-connected components are never closer than d2 = 4, so 1 could never find anything and is refused."""
    if isinstance(G, (bool, np.bool_)) or not isinstance(G, (int, np.integer)) or not 2 <= G <= GAP_MAX_RADIUS:
        raise ValueError(f"{what} is a whole number 2 .. {GAP_MAX_RADIUS}, got {G!r}")
    return int(G)


def gap_target(to, what="to"):
    """what an end may bridge to: "any" centerline pixel of another crack, or only an "end" (an end or an isolated pixel)"""
    if not isinstance(to, str) or to not in GAP_TO:
        raise ValueError(f'{what} is "any" or "end", got {to!r}')
    return to


def _gap_planes(topo, labels):
    labels = _labels(labels)                                 # a host tensor is refused before anything is moved
    topo = _topo(topo)
    if tuple(labels.shape) != tuple(topo.shape) or labels.device != topo.device:
        raise ValueError(f"labels {tuple(labels.shape)} has one value per topo byte {tuple(topo.shape)}, on the same device")
    return topo, labels


def _gap_map(t, like, what):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.dim() == 3 and (like is None or tuple(t.shape) == tuple(like.shape))):
        raise ValueError(f"{what} is the int32 device tensor [N, H, W] of endpoint_gaps")
    return t.contiguous()


def endpoint_gaps(topo, labels, max_gap, to="any"):
    """For every end of the centerline the nearest centerline pixel of another crack (csrc/gaps.hip): (gap_q, gap_d2), int32
    device tensors [N, H, W], for ``skeleton_topology``'s topo and an int32 device label map [N, H, W] (``label_components``', or any other:
    two pixels belong to the same crack iff their labels are equal and non-zero).  A source is a pixel of class end or isolated with a
    label; a candidate for it a pixel q of the same plane with a class (``to`` = "end": an end or an isolated pixel), a label other than
    the source's and d2 = |q - p|^2 <= ``max_gap``^2 (``gap_radius``).  gap_q is the linear index y W + x of the candidate with the smallest
    (d2, q) -- the nearest, among equals the first in raster order -- and gap_d2 its d2; -1 and 0 at every other pixel.  Planes are
    independent and nothing is read by the host."""
    G, to = gap_radius(max_gap), gap_target(to)
    topo, labels = _gap_planes(topo, labels)
    L.load()
    N, H, W = topo.shape
    gap_q, gap_d2 = (torch.empty(N, H, W, dtype=torch.int32, device=topo.device) for _ in range(2))
    with torch.cuda.device(topo.device):
        L.call("csbsr_endpoint_gaps", _ptr(topo), _ptr(labels), N, H, W, G, int(to == "end"), _ptr(gap_q), _ptr(gap_d2), L.stream(topo.device))
    return gap_q, gap_d2


def gap_table(topo, labels, gap_q, gap_d2):
    """One row per gap of ``endpoint_gaps``: int32 device tensor [M, 8] = ``GAP_COLUMNS``, in raster order of the source p, plane by plane.
    p and q are linear indices within the plane, label_p / label_q ``labels`` there, class_q the class of the target (1 isolated, 2 end,
    3 path, 4 junction) and mutual 1 where the gap of q is p.  Built with indexing on the device; nothing is read by the host."""
    topo, labels = _gap_planes(topo, labels)
    gap_q, gap_d2 = _gap_map(gap_q, labels, "gap_q"), _gap_map(gap_d2, labels, "gap_d2")
    N, H, W = labels.shape
    fq = gap_q.view(N, H * W)
    at = torch.nonzero(fq >= 0)
    n, p = at[:, 0], at[:, 1]
    q = fq[n, p].long()
    fl = labels.view(N, H * W)
    cols = [n, p, q, gap_d2.view(N, H * W)[n, p], fl[n, p], fl[n, q], topo.view(N, H * W)[n, q] & 7, fq[n, q] == p]
    return torch.stack([c.to(torch.int64) for c in cols], 1).to(torch.int32)


def gap_groups(labels, gap_q):
    """The cracks joined by the gaps: int32 device tensor [N, H, W], 0 where ``labels`` is 0, else the smallest label of the pixel's group --
    the labels connected by the transitive closure of "a gap leads from a pixel of label a to a pixel of label b" (csbsr_gap_groups: the
    lock-free union-find of the component labelling over the labels).  With ``label_components``' labels (1 + the first pixel's linear
    index) that is the group's first pixel in raster order.  The labels lie in 1 .. H W.  Nothing is read by the host."""
    labels = _labels(labels)
    gap_q = _gap_map(gap_q, labels, "gap_q")
    L.load()
    N, H, W = labels.shape
    parent, groups = (torch.empty(N, H, W, dtype=torch.int32, device=labels.device) for _ in range(2))
    with torch.cuda.device(labels.device):
        L.call("csbsr_gap_groups", _ptr(labels), _ptr(gap_q), N, H, W, _ptr(parent), _ptr(groups), L.stream(labels.device))
    return groups


def draw_bridges(gap_q):
    """The bridges of the gaps: uint8 device tensor [N, H, W] of 0 / 1 with the 8-connected Bresenham line of every gap (p, gap_q[p]), drawn
    from the end with the smaller linear index, both ends included (csbsr_gap_draw).  The bridged skeleton is skeleton | bridges."""
    gap_q = _gap_map(gap_q, None, "gap_q")
    L.load()
    N, H, W = gap_q.shape
    out = torch.empty(N, H, W, dtype=torch.uint8, device=gap_q.device)
    with torch.cuda.device(gap_q.device):
        L.call("csbsr_gap_draw", _ptr(gap_q), N, H, W, _ptr(out), L.stream(gap_q.device))
    return out


def gap_length(d2):
    """the length of a gap in pixels, fp64 on the host: sqrt(d2) (ints, NumPy arrays or tensors; a Python float for a scalar)"""
    g = np.sqrt(_host_ints(d2).astype(np.float64))
    return float(g) if g.ndim == 0 else g


def _gap_rows(rows):
    rows = _host_ints(rows).astype(np.int64)
    if rows.ndim != 2 or rows.shape[1] != len(GAP_COLUMNS):
        if rows.size:
            raise ValueError(f"rows is [M, {len(GAP_COLUMNS)}], the rows of gap_table, got shape {rows.shape}")
        rows = rows.reshape(0, len(GAP_COLUMNS))
    return rows


def gap_group_of(rows):
    """label -> the smallest label of its group, for the labels that the rows of ONE plane name (a union-find on the host)"""
    parent = {}

    def find(i):
        while parent.setdefault(i, i) != i:
            i = parent[i]
        return i
    for a, b in _gap_rows(rows)[:, 4:6].tolist():
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return {k: find(k) for k in parent}


def summarize_gaps(rows, n_cracks):
    """The gap figures of ONE plane from its rows of ``gap_table``, fp64 on the host: n_gaps (the rows), n_mutual (the rows whose target's
    gap leads back: a mutual pair is two of them), n_end_to_end (the target is an end or an isolated pixel), n_end_to_side (it is a path or
    a junction pixel), gap_length_px (the sum of ``gap_length``, a mutual pair counted once), max_gap_px, and n_cracks_bridged = ``n_cracks``
    minus the joins the gaps make: the groups among ``n_cracks`` cracks that include every label of the rows."""
    rows = _gap_rows(rows)
    if isinstance(n_cracks, (bool, np.bool_)) or not isinstance(n_cracks, (int, np.integer)) or n_cracks < 0:
        raise ValueError(f"n_cracks is a whole number >= 0, got {n_cracks!r}")
    once = (rows[:, 7] == 0) | (rows[:, 1] < rows[:, 2])
    ee = int(((rows[:, 6] == TOPO_ISOLATED) | (rows[:, 6] == TOPO_END)).sum())
    group = gap_group_of(rows)
    return {"n_gaps": int(rows.shape[0]), "n_mutual": int((rows[:, 7] != 0).sum()), "n_end_to_end": ee, "n_end_to_side": int(rows.shape[0]) - ee,
            "gap_length_px": float(np.sqrt(rows[once, 3].astype(np.float64)).sum()),
            "max_gap_px": float(np.sqrt(np.float64(rows[:, 3].max()))) if rows.shape[0] else 0.0,
            "n_cracks_bridged": int(n_cracks) - (len(group) - len(set(group.values())))}


class IoU:
    """estimate_metrics.py:64-84 for binary maps (threshold 0.5)."""
    name = "IoU"

    def __init__(self, th=0.5):
        self.th = 0.5

    def __call__(self, output, target):
        if output.dim() == 4 and output.shape[1] > 1:       # already a stack of binarised maps [B,T,H,W]
            B, T = output.shape[:2]
            outs = [iou_sweep(output[:, t:t + 1], target, [self.th]) for t in range(T)]
            return torch.cat(outs, 1).cpu().numpy()
        return iou_sweep(output, target, [self.th]).cpu().numpy()


# ------------------------------------------------------------------------------------------- surface distances (HD / MSD)
# calc_distance_metrics (model/engine/inference.py:293-336) on top of model/utils/metrics/surface_distance, 2-D, spacing (1, 1).  The device
# (csrc/surface_distance.hip) delivers, per (image, threshold, direction), integer counts keyed by  d^2 * 4 + length class ; everything
# floating-point happens below, in fp64, as a function of those integers alone.

def contour_class_table():
    """length class (0 .. 3) of each of the 16 neighbour codes  8 m[i-1,j-1] + 4 m[i-1,j] + 2 m[i,j-1] + m[i,j]  of a corner: marching
    squares joins the midpoints of the cell edges whose two pixels differ -- one or three pixels set: one diagonal between adjacent edge
    midpoints (class 1); two adjacent pixels: one straight segment across the cell (2); two opposite pixels: two diagonals (3)."""
    cls = np.zeros(16, np.int64)
    for code in range(16):
        n = bin(code).count("1")
        if n in (1, 3):
            cls[code] = 1
        elif n == 2:
            cls[code] = 3 if code in (0b1001, 0b0110) else 2
    return cls


_HALF_DIAG = float(np.hypot(0.5, 0.5))                       # midpoint of one cell edge to the midpoint of an adjacent one
CLASS_LENGTH = np.array([0.0, _HALF_DIAG, 1.0, 2.0 * _HALF_DIAG])


def contour_length_table():
    """contour length of each neighbour code at unit spacing (fp64 [16])."""
    return CLASS_LENGTH[contour_class_table()]


# a bin's total length is  count * (u * sqrt(1/2) + v)  with integer (u, v): the running sums stay integers until one final fp64 expression
_CLASS_U = np.array([0, 1, 0, 2], np.int64)
_CLASS_V = np.array([0, 0, 1, 0], np.int64)


def _finish_tables(table, keys, counts, ntab, frac):
    """per table t < ntab, from its integer bins (rows with table == t, any order, >= 1 row each): the percentile distance -- the first bin,
    in (d^2, class) order, whose cumulative contour length reaches ``frac`` of the table's -- , sum d * len and sum len (fp64 [ntab] each)."""
    table, keys, counts = (np.asarray(a, np.int64) for a in (table, keys, counts))
    order = np.argsort((table << 32) | keys)                  # by (table, key); keys are < 2^31
    t, k, c = table[order], keys[order], counts[order]
    start = np.searchsorted(t, np.arange(ntab))
    assert np.array_equal(t[start], np.arange(ntab)), "every table needs at least one bin"
    last = np.append(start[1:], len(t)) - 1
    cls = k & 3
    d = np.sqrt((k >> 2).astype(np.float64))
    u, v = c * _CLASS_U[cls], c * _CLASS_V[cls]
    cu, cv = np.cumsum(u), np.cumsum(v)
    cu, cv = cu - (cu[start] - u[start])[t], cv - (cv[start] - v[start])[t]          # running sums within each table
    cum = cu * _HALF_DIAG + cv
    total = cum[last]
    reached = np.where(cum / total[t] >= frac, np.arange(len(t)), len(t))
    idx = np.minimum(np.minimum.reduceat(reached, start), last)
    return d[idx], np.add.reduceat(d * (u * _HALF_DIAG + v), start), total


def surface_metrics_from_counts(gt_to_pred, pred_to_gt, percent=50.0, max_img_len=0):
    """HD(percent) and MSD of one (image, threshold) cell from its integer counts.  Each direction is (keys, counts): keys = d^2 * 4 + length
    class of the border corners of one contour against the other, in any order (distinct or not), counts their multiplicities; an empty pair
    = that contour has no border corner.  Returns (hd, msd, hd_outlier, msd_outlier) with the reference's degenerate rules: neither contour
    -> 0; exactly one -> max_img_len and an outlier count each."""
    ng, npd = len(gt_to_pred[0]), len(pred_to_gt[0])
    if ng == 0 and npd == 0:
        return 0.0, 0.0, 0, 0
    if ng == 0 or npd == 0:
        return float(max_img_len), float(max_img_len), 1, 1
    table = np.concatenate([np.zeros(ng, np.int64), np.ones(npd, np.int64)])
    perc, sdl, tot = _finish_tables(table, np.concatenate([gt_to_pred[0], pred_to_gt[0]]), np.concatenate([gt_to_pred[1], pred_to_gt[1]]),
                                    2, percent / 100.0)
    return float(perc.max()), float(sdl[0] / tot[0] + sdl[1] / tot[1]) / 2, 0, 0


def _pow2_above(n):
    return 1 << int(2 * n - 1).bit_length() if n > 0 else 0            # a power of two >= 2 n: load factor <= 1/2


def surface_distance_sweep(segment_preds, masks, thresholds, percent=50.0, workspace_bytes=256 << 20):
    """HD(percent) and MSD between the contours of (masks > 0.5) and (segment_preds - t > 0) for every threshold:
    dict(hd [B,T] float64, msd [B,T] float64, hd_outliers int, msd_outliers int) -- calc_distance_metrics of the reference (whose percent is
    50 although it prints "HD95"; its max_img_len for degenerate cells is the WIDTH, np.max(preds.shape[3:])).  ``workspace_bytes`` bounds
    the per-chunk device workspace (column-scan planes + count tables); the thresholds of an image are processed in chunks that fit."""
    L.load()
    p = _dev32(segment_preds)
    m = _dev32(masks, p)
    H, W = int(p.shape[-2]), int(p.shape[-1])
    p, m = p.reshape(-1, H, W), m.reshape(-1, H, W)
    B = p.shape[0]
    assert m.shape[0] == B, "one mask per prediction map"
    th = torch.tensor([float(t) for t in thresholds], dtype=torch.float32)          # == torch.Tensor(thresholds): fp32 roundings
    assert bool((th[1:] > th[:-1]).all()), "thresholds must ascend"
    T = th.numel()
    dev = p.device
    th = th.to(dev)
    st = L.stream(p.device)
    ncorner = (H + 1) * (W + 1)
    i32, u8 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.uint8, device=dev)
    lvl, gt = torch.empty(H * W, **u8), torch.empty(H * W, **u8)
    gcol0, dgt = torch.empty(ncorner, dtype=torch.int16, device=dev), torch.empty(ncorner, **i32)
    hd, msd = np.zeros((B, T)), np.zeros((B, T))
    hd_out = msd_out = 0
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64))
    for b in range(B):
        counts, rowflag = torch.zeros(T + 2, **i32), torch.zeros(H + 1, **i32)
        L.call("csbsr_surface_prepare", _ptr(p[b]), _ptr(m[b]), _ptr(th), H, W, T, _ptr(lvl), _ptr(gt), _ptr(counts), _ptr(rowflag),
               _ptr(gcol0), _ptr(dgt), st)
        c = counts.cpu().numpy().astype(np.int64)
        n_gt, n_pred = int(c[0]), np.cumsum(c[1:T + 1])
        caps = np.zeros((T, 2), np.int64)
        for j in range(T):
            if n_gt > 0 and n_pred[j] > 0:
                caps[j] = _pow2_above(n_gt), _pow2_above(int(n_pred[j]))
            else:
                one = (np.zeros(1, np.int64), np.ones(1, np.int64))
                hd[b, j], msd[b, j], ho, mo = surface_metrics_from_counts(one if n_gt > 0 else empty, one if n_pred[j] > 0 else empty,
                                                                          percent, W)
                hd_out += ho
                msd_out += mo
        nrows = np.where(caps[:, 0] > 0, n_gt + n_pred, 0)       # distinct bins of a cell <= its border corners
        need = 2 * ncorner + 8 * caps.sum(1) + 12 * nrows     # bytes per threshold: a uint16 plane, (key, count) per slot, compacted rows
        j0 = 0
        while j0 < T:
            if caps[j0, 0] == 0:
                j0 += 1
                continue
            nj, used = 0, 0
            while j0 + nj < T and (nj == 0 or used + need[j0 + nj] <= workspace_bytes):
                used += need[j0 + nj]
                nj += 1
            if used > workspace_bytes:
                raise L.CsbsrHipError(f"surface_distance_sweep: one threshold of a {H}x{W} image needs {used} bytes of workspace, "
                                      f"workspace_bytes is {workspace_bytes}")
            cap = caps[j0:j0 + nj].reshape(-1)
            off = np.concatenate([[0], np.cumsum(cap)[:-1]])
            total, max_rows = int(cap.sum()), int(nrows[j0:j0 + nj].sum())
            assert total < 2 ** 31 and max_rows < 2 ** 31
            t_off = torch.from_numpy(off.astype(np.int32)).to(dev)
            t_cap = torch.from_numpy(cap.astype(np.int32)).to(dev)
            keys, cnts = torch.full((total,), -1, **i32), torch.zeros(total, **i32)
            rows, meta = torch.empty(max_rows, 3, **i32), torch.zeros(2, **i32)
            gcol = torch.empty(nj * ncorner, dtype=torch.int16, device=dev)
            L.call("csbsr_surface_gather", _ptr(lvl), _ptr(gt), _ptr(dgt), _ptr(rowflag), H, W, j0, nj, _ptr(gcol), _ptr(t_off), _ptr(t_cap),
                   _ptr(keys), _ptr(cnts), int(cap.max()), _ptr(rows), max_rows, _ptr(meta), st)
            err, n = meta.cpu().tolist()
            if err != 0:
                raise L.CsbsrHipError("surface_distance_sweep: a count table overflowed")
            r = rows[:n].cpu().numpy()
            live = np.nonzero(cap[0::2] > 0)[0]                # the chunk's non-degenerate cells; their tables renumbered 0 .. 2 * len - 1
            renum = np.full(2 * nj, -1, np.int64)
            renum[2 * live], renum[2 * live + 1] = 2 * np.arange(len(live)), 2 * np.arange(len(live)) + 1
            perc, sdl, tot = _finish_tables(renum[r[:, 0]], r[:, 1], r[:, 2], 2 * len(live), percent / 100.0)
            hd[b, j0 + live] = np.maximum(perc[0::2], perc[1::2])
            msd[b, j0 + live] = (sdl[0::2] / tot[0::2] + sdl[1::2] / tot[1::2]) / 2
            j0 += nj
    return dict(hd=hd, msd=msd, hd_outliers=int(hd_out), msd_outliers=int(msd_out))
