"""Patch-tiled evaluation step on the device: the body of ``inference_for_ss``
(model/engine/inference.py:76-119) for one batch of test images -- patches through JointModel, stitch, clip, PSNR / SSIM of the SR
image, PSNR of the kernel, and the IoU of the segmentation map at every threshold 0.01 .. 0.99 -- without the [B,99,H,W] broadcast
tensor and the host numpy reductions.  ``evaluate_dataset`` runs it over a whole HBM-resident test set (csbsr_amd/data/resident_test.py) and
returns the reference's final report, with the saved images and masks leaving the device as uint8 (csrc/eval_io.hip); on request
(``pr_tolerance``) also the tolerance-matched precision / recall / F of the map over the same thresholds (csrc/pr_sweep.hip), and
(``cldice_threshold``) the centerline Dice of the map at one threshold (csrc/skeleton.hip), neither of which the reference computes.
``predict_dataset`` is the other driver of test.py, ``inference_tti_building`` (inference.py:210-273): unlabeled LR images of any size out
of an HBM pool (csbsr_amd/data/resident_predict.py), tiled, run and stitched on the device; on request (``measure_threshold``) with the
crack's area, centerline length and mean width per image, and (``min_crack_px``) with the small blobs dropped and the same numbers per
connected crack (csrc/components.hip), (``width_radius``) with the local width at every centerline pixel (csrc/width.hip), and
(``topology``) with the ends, junctions, loops and geodesic length of the centerline (csrc/topology.hip), and (``prune_spur_px``) with the
centerline's short side branches removed before any of that is measured (csrc/prune.hip), and (``branches``) with one row per centerline
segment between junctions (csrc/branches.hip), and (``polylines``) with every segment's pixels in order from end to end
(csrc/polylines.hip), and (``simplify_px``) with those polylines simplified to their vertices (csrc/simplify.hip), and (``bridge_gap_px``)
with the gaps between the ends of one crack and the nearest other crack, the cracks they join and the bridges drawn (csrc/gaps.hip)."""
import csv
import gc
import json
import math
import os

import numpy as np
import torch

from . import _lib as L
from .data.patch_sampler import JointPatch
from .engine import _ptr
from .utils.estimate_metrics import psnr_ssim, iou_sweep, surface_distance_sweep, pr_sweep, pr_tol2
from .utils.estimate_metrics import skeletonize, centerline_counts, cldice_scores, summarize_cldice, unit_threshold
from .utils.estimate_metrics import label_components, component_min_px, _component_sums, _keep_from_sums, _table_from_sums
from .utils.estimate_metrics import skeleton_width, summarize_width_hist, width_from_d2, _component_width, _width_columns
from .utils.estimate_metrics import width_radius as _width_radius
from .utils.estimate_metrics import skeleton_topology, summarize_topology, geodesic_length, orientation_shares, euler_number, mean_width_geodesic
from .utils.estimate_metrics import _junction_labels, _count_roots, _component_topology, _topology_columns, TOPO_COUNTS, TOPO_ACC
from .utils.estimate_metrics import prune_spurs, spur_length
from .utils.estimate_metrics import label_branches, branch_table, branch_kinds, BRANCH_COLUMNS, BRANCH_KINDS, _SQRT2
from .utils.estimate_metrics import order_branches, branch_polylines, arc_position, _diag_along
from .utils.estimate_metrics import simplify_tolerance, simplify_polylines, polyline_length
from .utils.estimate_metrics import gap_radius, gap_target, endpoint_gaps, gap_table, gap_groups, draw_bridges, gap_length, gap_group_of
from .utils.estimate_metrics import summarize_gaps, GAP_COLUMNS, TOPO_ISOLATED, TOPO_END

THRESHOLDS = [i * 0.01 for i in range(1, 100)]           # inference.py:50


def _kernel_for_psnr(model, kernel_preds, kernel_targets):
    """The kernel estimate the kernel-PSNR column is taken on.  A MODEL.SR == "bicubic" model has none: its ``kernel_preds`` are zeros
    of the DUMMY kernel's shape, and the column is the PSNR of a zero kernel of the target's shape -- what the reference computes whenever
    its shapes allow."""
    if getattr(model, "sr_model", None) == "bicubic" and kernel_preds.shape != kernel_targets.shape:
        return torch.zeros_like(kernel_targets, dtype=kernel_preds.dtype)
    return kernel_preds


@torch.no_grad()
def evaluate_batch(model, imgs, img_unfold_shape, seg_unfold_shape, sr_targets, masks, kernel_targets, ksize, thresholds=THRESHOLDS,
                   surface_distance=False, pr_tolerance=None, cldice_threshold=None):
    """imgs [B, nPatch, 3, h, w] LR patches (as CrackDataSetTest delivers them), kernel_targets [B, nPatch, K, K];
    returns dict(sr_preds, segment_preds, psnr [B], ssim [B], kernel_psnr [B*nPatch], iou [B, T]) -- numpy arrays for the metrics.
    surface_distance=True adds hd [B, T], msd [B, T] (float64) and the counters hd_outliers, msd_outliers of calc_distance_metrics
    (inference.py:293-336) at the same thresholds.  pr_tolerance = a radius in pixels adds pr_counts [B, 4, T] (int64), the tolerance-matched
    precision / recall counts of ``pr_sweep`` (scores: ``pr_scores``, ``summarize_pr``); None adds nothing.  cldice_threshold = a float
    strictly inside (0, 1) adds cl_counts [B, 4] (int64), the centerline counts of ``centerline_counts`` at that one threshold (scores:
    ``cldice_scores``, ``summarize_cldice``); None adds nothing."""
    if pr_tolerance is not None:
        pr_tol2(pr_tolerance)
    if cldice_threshold is not None:
        cldice_threshold = unit_threshold(cldice_threshold, "cldice_threshold")
    joint = JointPatch()
    imgs = imgs.view(-1, *imgs.shape[2:])
    kernel_targets = kernel_targets.view(-1, 1, *kernel_targets.shape[2:])
    dummy = torch.zeros((imgs.shape[0], 1, ksize, ksize))
    sr_preds, segment_preds, kernel_preds = model(imgs, dummy, sr_targets=sr_targets)
    sr_preds = joint(sr_preds, img_unfold_shape)
    segment_preds = joint(segment_preds, seg_unfold_shape)
    sr_preds = sr_preds.clamp(0, 1)
    kernel_preds = kernel_preds.clamp(0, 1)
    ps, ss = psnr_ssim(sr_preds, sr_targets)
    kps, _ = psnr_ssim(_kernel_for_psnr(model, kernel_preds, kernel_targets), kernel_targets)
    iou = iou_sweep(segment_preds, masks, thresholds)
    out = dict(sr_preds=sr_preds, segment_preds=segment_preds, kernel_preds=kernel_preds, psnr=ps.cpu().numpy(), ssim=ss.cpu().numpy(),
               kernel_psnr=kps.cpu().numpy(), iou=iou.cpu().numpy())
    if surface_distance:
        out.update(surface_distance_sweep(segment_preds, masks, thresholds))
    if pr_tolerance is not None:
        out["pr_counts"] = pr_sweep(segment_preds, masks, thresholds, pr_tolerance).cpu().numpy().astype(np.int64)
    if cldice_threshold is not None:
        out["cl_counts"] = centerline_counts(segment_preds, masks, cldice_threshold).cpu().numpy().astype(np.int64)
    return out


# ------------------------------------------------------------------------------------------------ whole-test-set evaluation
SAVE_THRESHOLD_IDX = [0] + [9 + i * 10 for i in range(9)] + [98]      # inference.py:53: the thresholds whose binary masks are saved
CLASSIFICATION_IDX = 49                                              # inference.py:123: accuracy / sensitivity / specificity at 0.50
_SLOTS = 3         # pinned read-back ring: a slot is rewritten three batches after its copies were enqueued, long after it was encoded


def stitch_clip_u8(patches, unfold_shape, clip, want_f32=True, want_u8=False):
    """csbsr_stitch_clip_u8 on the model's patch batch [B * nH * nW, C, ph, pw] with the 1-D ``unfold_shape`` of the loader:
    (fp32 [B,C,H,W] or None, uint8 [B,H,W,C] or None) -- JointPatch, the masked clip (``clip``) and ToPILImage's quantisation."""
    s = [int(v) for v in unfold_shape]
    if s[1] != 1:
        raise L.CsbsrHipError(f"stitch_clip_u8: the channel axis is not split on the evaluation path (unfold_shape[1] = {s[1]})")
    nH, nW, Cc, ph, pw = s[2:]
    if not patches.is_cuda:
        raise L.CsbsrHipError("stitch_clip_u8 needs the patches on a GPU: csbsr_amd has no fallback path")
    p = patches.to(torch.float32).contiguous()
    if p.numel() % (nH * nW * Cc * ph * pw) or p.numel() == 0:
        raise ValueError(f"{tuple(patches.shape)} is not a whole number of images of unfold shape {s[1:]}")
    B = p.numel() // (nH * nW * Cc * ph * pw)
    f32 = torch.empty(B, Cc, nH * ph, nW * pw, dtype=torch.float32, device=p.device) if want_f32 else None
    u8 = torch.empty(B, nH * ph, nW * pw, Cc, dtype=torch.uint8, device=p.device) if want_u8 else None
    with torch.cuda.device(p.device):
        L.call("csbsr_stitch_clip_u8", _ptr(p), B, Cc, nH, nW, ph, pw, int(bool(clip)), None if f32 is None else _ptr(f32),
               None if u8 is None else _ptr(u8), L.stream(p.device))
    return f32, u8


def stitch_tiles_u8(patches, tiles, offsets, dims, clip, out_f32=None, out_u8=None):
    """csbsr_stitch_tiles_u8: the owned rectangle of every patch of fp32 ``patches`` [N, C, PH, PW] into the output pools, in place, by the
    int32 device table ``tiles`` [N, 8] = (image, dst_y, dst_x, src_y, src_x, th, tw, 0) over the int64 ``offsets`` [n] and int32 ``dims``
    [n, 2] tables of the output images (include/csbsr_hip.h).  ``out_f32``: flat fp32 pool, planar per image; ``out_u8``: flat uint8 pool,
    interleaved per image; at least one.  The caller sizes the pools for the tables and keeps the image column inside them."""
    if not patches.is_cuda:
        raise L.CsbsrHipError("stitch_tiles_u8 needs the patches on a GPU: csbsr_amd has no fallback path")
    if out_f32 is None and out_u8 is None:
        raise L.CsbsrHipError("stitch_tiles_u8: no output pool")
    p = patches.to(torch.float32).contiguous()
    if p.dim() != 4 or tuple(tiles.shape) != (p.shape[0], 8) or tiles.dtype != torch.int32 or not tiles.is_contiguous():
        raise ValueError(f"patches {tuple(patches.shape)} need one contiguous int32 row of 8 each: tiles {tuple(tiles.shape)} {tiles.dtype}")
    if offsets.dtype != torch.int64 or dims.dtype != torch.int32 or dims.shape != (offsets.numel(), 2) or not dims.is_contiguous():
        raise ValueError("offsets must be int64 [n] and dims contiguous int32 [n, 2]")
    for o, dt in ((out_f32, torch.float32), (out_u8, torch.uint8)):
        if o is not None and (o.dtype != dt or not o.is_contiguous() or o.device != p.device):
            raise ValueError(f"an output pool must be a contiguous {dt} tensor on {p.device}")
    N, Cc, PH, PW = p.shape
    with torch.cuda.device(p.device):
        L.call("csbsr_stitch_tiles_u8", _ptr(p), N, Cc, PH, PW, _ptr(tiles), _ptr(offsets), _ptr(dims), int(bool(clip)),
               None if out_f32 is None else _ptr(out_f32), None if out_u8 is None else _ptr(out_u8), L.stream(p.device))


def threshold_planes_u8(pred, thresholds32):
    """csbsr_threshold_planes_u8: uint8 [N, S, *pred.shape[1:]] = 255 where pred - t_s > 0 (fp32), for fp32 device tensors pred [N, ...] and
    thresholds32 [S], 1 <= S <= 16."""
    if not pred.is_cuda:
        raise L.CsbsrHipError("threshold_planes_u8 needs the map on a GPU: csbsr_amd has no fallback path")
    p = pred.to(torch.float32).contiguous()
    th = thresholds32.to(p.device, torch.float32).contiguous()
    N, S = p.shape[0], th.numel()
    out = torch.empty(N, S, *p.shape[1:], dtype=torch.uint8, device=p.device)
    with torch.cuda.device(p.device):
        L.call("csbsr_threshold_planes_u8", _ptr(p), _ptr(th), N, p[0].numel(), S, _ptr(out), L.stream(p.device))
    return out


def summarize(psnr, ssim, kernel_psnr, iou, hd=None, msd=None):
    """The final report of inference_for_ss (inference.py:170-190 and plot_metrics_th) from the per-image scores, in float64: means over
    everything, and the best threshold of the mean-over-images curve (IoU_max = max_t mean_n, HD95_min = min_t mean_n) -- not the mean of
    per-image optima."""
    f = lambda a: np.asarray(a, dtype=np.float64)
    out = {"PSNR_mean": float(np.mean(f(psnr))), "SSIM_mean": float(np.mean(f(ssim))), "PSNR(Kernel)_mean": float(np.mean(f(kernel_psnr))),
           "AIU_mean": float(np.mean(f(iou))), "IoU_max": float(np.max(np.mean(f(iou), axis=0)))}
    if hd is not None:
        out.update({"HD95_mean": float(np.mean(f(hd))), "MSD_mean": float(np.mean(f(msd))), "HD95_median": float(np.median(f(hd))),
                    "MSD_median": float(np.median(f(msd))), "HD95_min": float(np.min(np.mean(f(hd), axis=0)))})
    return out


def write_iou_log(path, iou, thresholds, fnames):
    """iou_log.csv (inference.py:287-289): one row per image, one column per threshold, the header row starting with an empty cell like a
    DataFrame's index column.  Values are written with the shortest text that reads back to the same fp32; the file is not byte-identical
    to pandas' output."""
    iou = np.asarray(iou, dtype=np.float32)
    assert iou.shape == (len(fnames), len(thresholds))
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow([""] + [repr(float(t)) for t in thresholds])
        for name, row in zip(fnames, iou):
            w.writerow([name] + [str(v) for v in row])


def classification_counts(segment_preds, masks, threshold32):
    """int64 device [B, 4] = (tp, tn, ground pixels, non-ground pixels) of (segment_preds - t > 0) against the mask cast to an integer the
    way get_retinal_seg_metrics casts ``mask / 255`` to int16: 1 only where the mask byte is 255."""
    B = segment_preds.shape[0]
    seg = (segment_preds.reshape(B, -1) - threshold32 > 0)
    gt = masks.reshape(B, -1).to(torch.int64) != 0
    return torch.stack([(seg & gt).sum(1), (~seg & ~gt).sum(1), gt.sum(1), (~gt).sum(1)], dim=1)


def classification_scores(counts):
    """(acc, sens, spec) float64 [N] from the integer counts (retinal_metrics.py:30-62); 0 / 0 stays NaN as numpy leaves it."""
    c = np.asarray(counts, dtype=np.int64)
    tp, tn, ng, nn = (c[:, i].astype(np.float64) for i in range(4))
    with np.errstate(divide="ignore", invalid="ignore"):
        acc, sens, spec = (tp + tn) / (ng + nn), tp / ng, tn / nn
    sens[sens == np.inf] = 1
    spec[spec == np.inf] = 1
    return acc, sens, spec


# ------------------------------------------------------------------------------------------------ precision / recall / F
def pr_scores(counts):
    """(precision, recall, f) float64 [N, T] from the integer counts [N, 4, T] = (n_pred, tp_pred, tp_gt, n_gt) of ``pr_sweep``:
    precision = tp_pred / n_pred, recall = tp_gt / n_gt, f = 2 P R / (P + R).  Fixed conventions for the degenerate cells: nothing predicted
    (n_pred = 0) -> precision 1; no ground truth (n_gt = 0) -> recall 1; P + R = 0 -> f 0."""
    c = np.asarray(counts, dtype=np.int64)
    assert c.ndim == 3 and c.shape[1] == 4, f"counts are [N, 4, T], got {c.shape}"
    n_pred, tp_pred, tp_gt, n_gt = (c[:, i].astype(np.float64) for i in range(4))
    p = np.where(n_pred > 0, tp_pred / np.maximum(n_pred, 1.0), 1.0)
    r = np.where(n_gt > 0, tp_gt / np.maximum(n_gt, 1.0), 1.0)
    f = np.where(p + r > 0, 2.0 * p * r / np.where(p + r > 0, p + r, 1.0), 0.0)
    return p, r, f


def summarize_pr(counts, thresholds):
    """The summaries the crack / edge-detection literature reports, from the counts [N, 4, T] of ``pr_sweep`` (scores by ``pr_scores``):
    ODS (optimal dataset scale) = max over thresholds of the F of the counts summed over the images, reached at ODS_threshold (the first
    such threshold) with P_at_ODS, R_at_ODS; OIS (optimal image scale) = the mean over images of each image's best F; AP = the area under
    the dataset precision-over-recall curve, by the trapezoid rule across the T points as they are (no extrapolation to recall 0 or 1).
    The dataset recall never grows with the threshold index, so every trapezoid has a non-negative width."""
    c = np.asarray(counts, dtype=np.int64)
    assert c.ndim == 3 and c.shape[1] == 4 and c.shape[2] == len(thresholds) and c.shape[0] >= 1
    p, r, f = (a[0] for a in pr_scores(c.sum(axis=0, keepdims=True)))
    j = int(np.argmax(f))
    ap = float(np.sum((r[:-1] - r[1:]) * (p[:-1] + p[1:]) * 0.5))
    return {"ODS": float(f[j]), "ODS_threshold": float(thresholds[j]), "OIS": float(np.mean(np.max(pr_scores(c)[2], axis=1))), "AP": ap,
            "P_at_ODS": float(p[j]), "R_at_ODS": float(r[j])}


def write_pr_log(path, counts, thresholds, fnames):
    """pr_log.csv: per image three rows (P, R, F) of ``pr_scores``, one column per threshold; the header row starts with two empty cells
    (the image and the score columns).  Values are written with repr, the shortest text that reads back to the same fp64."""
    scores = pr_scores(counts)
    assert scores[0].shape == (len(fnames), len(thresholds))
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["", ""] + [repr(float(t)) for t in thresholds])
        for i, name in enumerate(fnames):
            for tag, a in zip("PRF", scores):
                w.writerow([name, tag] + [repr(float(v)) for v in a[i]])


# ------------------------------------------------------------------------------------------------ centerlines
def write_cldice_log(path, counts, fnames):
    """cldice_log.csv: one row per image -- the four counts of ``centerline_counts`` and the three scores of ``cldice_scores`` (repr: the
    shortest text that reads back to the same fp64)."""
    c = np.asarray(counts, dtype=np.int64)
    assert c.shape == (len(fnames), 4)
    tp, ts, cl = cldice_scores(c)
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["", "skel_pred", "skel_pred_in_gt", "skel_gt", "skel_gt_in_pred", "Tprec", "Tsens", "clDice"])
        for i, name in enumerate(fnames):
            w.writerow([name] + [int(v) for v in c[i]] + [repr(float(a[i])) for a in (tp, ts, cl)])


def mean_width(crack_px, skeleton_px):
    """crack_px / skeleton_px in fp64, 0.0 for an empty skeleton"""
    return float(crack_px) / float(skeleton_px) if skeleton_px else 0.0


def write_crack_stats(path, rows):
    """crack_stats.csv: (name, crack_px, skeleton_px, mean_width_px) per image"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(["name", "crack_px", "skeleton_px", "mean_width_px"])
        for name, crack, skel, width in rows:
            w.writerow([name, int(crack), int(skel), repr(float(width))])


INSTANCE_COLUMNS = ["name", "crack", "y", "x", "area_px", "length_px", "mean_width_px", "y0", "x0", "y1", "x1"]


def crack_instances(table_rows, W):
    """the ``cracks`` list of one image from its rows of ``component_table`` (plane, label, area_px, skeleton_px, y0, x0, y1, x1), in the
    table's order = raster order of the first pixel (y, x); length_px is the component's skeleton pixels, a length of 0 gives width 0.0"""
    out = []
    for _, label, area, length, y0, x0, y1, x1 in table_rows:
        y, x = divmod(int(label) - 1, W)
        out.append(dict(y=y, x=x, area_px=int(area), length_px=int(length), mean_width_px=mean_width(area, length),
                        bbox=(int(y0), int(x0), int(y1), int(x1))))
    return out


def write_crack_instances(path, rows):
    """crack_instances.csv: one row per kept crack -- ``rows`` = (name, the image's ``cracks`` list) per image; ``crack`` counts from 0
    within the image (repr: the shortest text that reads back to the same fp64)"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(INSTANCE_COLUMNS)
        for name, cracks in rows:
            for j, c in enumerate(cracks):
                w.writerow([name, j, c["y"], c["x"], c["area_px"], c["length_px"], repr(float(c["mean_width_px"])), *c["bbox"]])


def read_crack_instances(path):
    """what ``write_crack_instances`` wrote: (name, cracks) per image, in the file's order"""
    out = []
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if rows[0] != INSTANCE_COLUMNS:
        raise ValueError(f"{path}: not a crack_instances.csv header: {rows[0]}")
    for name, j, y, x, area, length, width, y0, x0, y1, x1 in rows[1:]:
        if not out or out[-1][0] != name:
            out.append((name, []))
        if int(j) != len(out[-1][1]):
            raise ValueError(f"{path}: crack {j} of {name} is out of order")
        out[-1][1].append(dict(y=int(y), x=int(x), area_px=int(area), length_px=int(length), mean_width_px=float(width),
                               bbox=(int(y0), int(x0), int(y1), int(x1))))
    return out


WIDTH_COLUMNS = ["name", "centerline_px", "saturated_px", "centerline_width_px", "median_width_px", "p95_width_px", "max_width_px", "y_widest",
                 "x_widest"]
INSTANCE_WIDTH_COLUMNS = ["name", "crack", "max_width_px", "y_widest", "x_widest"]


def _yx(widest):
    return ["", ""] if widest is None else [int(widest[0]), int(widest[1])]


def _widest(y, x):
    return None if y == "" else (int(y), int(x))


def write_crack_widths(path, rows):
    """crack_widths.csv: one row per image -- ``rows`` = (name, dict with WIDTH_COLUMNS' figures and ``widest`` = (y, x) or None); an empty
    skeleton leaves y_widest and x_widest empty"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(WIDTH_COLUMNS)
        for name, d in rows:
            w.writerow([name, int(d["centerline_px"]), int(d["saturated_px"])] + [repr(float(d[k])) for k in WIDTH_COLUMNS[3:7]] + _yx(d["widest"]))


def read_crack_widths(path):
    """what ``write_crack_widths`` wrote: (name, dict) per image, in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if rows[0] != WIDTH_COLUMNS:
        raise ValueError(f"{path}: not a crack_widths.csv header: {rows[0]}")
    out = []
    for name, n, sat, mean, med, p95, mx, y, x in rows[1:]:
        out.append((name, dict(centerline_px=int(n), saturated_px=int(sat), centerline_width_px=float(mean), median_width_px=float(med),
                               p95_width_px=float(p95), max_width_px=float(mx), widest=_widest(y, x))))
    return out


def write_crack_instance_widths(path, rows):
    """crack_instance_widths.csv: one row per kept crack -- ``rows`` = (name, the image's ``cracks`` list with max_width_px and widest) per
    image; ``crack`` is the numbering of crack_instances.csv"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(INSTANCE_WIDTH_COLUMNS)
        for name, cracks in rows:
            for j, c in enumerate(cracks):
                w.writerow([name, j, repr(float(c["max_width_px"]))] + _yx(c["widest"]))


def read_crack_instance_widths(path):
    """what ``write_crack_instance_widths`` wrote: (name, [dict(max_width_px, widest)]) per image, in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if rows[0] != INSTANCE_WIDTH_COLUMNS:
        raise ValueError(f"{path}: not a crack_instance_widths.csv header: {rows[0]}")
    out = []
    for name, j, mx, y, x in rows[1:]:
        if not out or out[-1][0] != name:
            out.append((name, []))
        if int(j) != len(out[-1][1]):
            raise ValueError(f"{path}: crack {j} of {name} is out of order")
        out[-1][1].append(dict(max_width_px=float(mx), widest=_widest(y, x)))
    return out


TOPOLOGY_CSV_COLUMNS = ["name", "endpoints", "junctions", "junction_px", "isolated_px", "loops", "h", "v", "d_se", "d_sw", "length_geodesic_px",
                        "share_h", "share_v", "share_se", "share_sw", "mean_width_geodesic_px"]
INSTANCE_TOPOLOGY_COLUMNS = ["name", "crack", "endpoints", "junctions", "loops", "h", "v", "d_se", "d_sw", "length_geodesic_px", "share_h",
                             "share_v", "share_se", "share_sw"]


def crack_topology(sums, length_px):
    """the topology keys of one crack from its nine sums of ``component_topology_table`` (end, junction_px, h, v, d_se, d_sw, q4, isolated,
    junctions) and its centerline pixels: the centerline of one crack is one component, so loops = 1 - chi (0 - chi = 0 without a centerline)"""
    end, _, h, v, dse, dsw, q4, _, junctions = (int(k) for k in sums)
    links = (h, v, dse, dsw)
    return dict(endpoints=end, junctions=junctions, loops=(1 if length_px else 0) - euler_number(length_px, links, q4), links=links,
                length_geodesic_px=geodesic_length(*links), orientation=orientation_shares(*links))


def write_crack_topology(path, rows):
    """crack_topology.csv: one row per image -- ``rows`` = (name, dict with the topology keys of ``predict_dataset``)"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(TOPOLOGY_CSV_COLUMNS)
        for name, d in rows:
            w.writerow([name] + [int(d[k]) for k in TOPOLOGY_CSV_COLUMNS[1:6]] + [int(k) for k in d["links"]] + [repr(float(d["length_geodesic_px"]))]
                       + [repr(float(k)) for k in d["orientation"]] + [repr(float(d["mean_width_geodesic_px"]))])


def read_crack_topology(path):
    """what ``write_crack_topology`` wrote: (name, dict) per image, in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if rows[0] != TOPOLOGY_CSV_COLUMNS:
        raise ValueError(f"{path}: not a crack_topology.csv header: {rows[0]}")
    out = []
    for r in rows[1:]:
        d = {k: int(v) for k, v in zip(TOPOLOGY_CSV_COLUMNS[1:6], r[1:6])}
        d.update(links=tuple(int(v) for v in r[6:10]), length_geodesic_px=float(r[10]), orientation=tuple(float(v) for v in r[11:15]),
                 mean_width_geodesic_px=float(r[15]))
        out.append((r[0], d))
    return out


def write_crack_instance_topology(path, rows):
    """crack_instance_topology.csv: one row per kept crack -- ``rows`` = (name, the image's ``cracks`` list with the topology keys) per image;
    ``crack`` is the numbering of crack_instances.csv"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(INSTANCE_TOPOLOGY_COLUMNS)
        for name, cracks in rows:
            for j, c in enumerate(cracks):
                w.writerow([name, j, int(c["endpoints"]), int(c["junctions"]), int(c["loops"])] + [int(k) for k in c["links"]]
                           + [repr(float(c["length_geodesic_px"]))] + [repr(float(k)) for k in c["orientation"]])


def read_crack_instance_topology(path):
    """what ``write_crack_instance_topology`` wrote: (name, [dict]) per image, in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if rows[0] != INSTANCE_TOPOLOGY_COLUMNS:
        raise ValueError(f"{path}: not a crack_instance_topology.csv header: {rows[0]}")
    out = []
    for r in rows[1:]:
        if not out or out[-1][0] != r[0]:
            out.append((r[0], []))
        if int(r[1]) != len(out[-1][1]):
            raise ValueError(f"{path}: crack {r[1]} of {r[0]} is out of order")
        out[-1][1].append(dict(endpoints=int(r[2]), junctions=int(r[3]), loops=int(r[4]), links=tuple(int(v) for v in r[5:9]),
                               length_geodesic_px=float(r[9]), orientation=tuple(float(v) for v in r[10:14])))
    return out


SPUR_COLUMNS = ["name", "skeleton_px", "spur_px"]
INSTANCE_SPUR_COLUMNS = ["name", "crack", "length_px", "spur_px"]


def write_crack_spurs(path, rows):
    """crack_spurs.csv: one row per image -- ``rows`` = (name, skeleton_px, spur_px): the centerline pixels that are left and those pruned"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(SPUR_COLUMNS)
        for name, skel, spur in rows:
            w.writerow([name, int(skel), int(spur)])


def read_crack_spurs(path):
    """what ``write_crack_spurs`` wrote: (name, skeleton_px, spur_px) per image, in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if rows[0] != SPUR_COLUMNS:
        raise ValueError(f"{path}: not a crack_spurs.csv header: {rows[0]}")
    return [(name, int(skel), int(spur)) for name, skel, spur in rows[1:]]


def write_crack_instance_spurs(path, rows):
    """crack_instance_spurs.csv: one row per kept crack -- ``rows`` = (name, the image's ``cracks`` list with length_px and spur_px) per
    image; ``crack`` is the numbering of crack_instances.csv"""
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(INSTANCE_SPUR_COLUMNS)
        for name, cracks in rows:
            for j, c in enumerate(cracks):
                w.writerow([name, j, int(c["length_px"]), int(c["spur_px"])])


def read_crack_instance_spurs(path):
    """what ``write_crack_instance_spurs`` wrote: (name, [dict(length_px, spur_px)]) per image, in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    if rows[0] != INSTANCE_SPUR_COLUMNS:
        raise ValueError(f"{path}: not a crack_instance_spurs.csv header: {rows[0]}")
    out = []
    for name, j, length, spur in rows[1:]:
        if not out or out[-1][0] != name:
            out.append((name, []))
        if int(j) != len(out[-1][1]):
            raise ValueError(f"{path}: crack {j} of {name} is out of order")
        out[-1][1].append(dict(length_px=int(length), spur_px=int(spur)))
    return out


BRANCH_CSV_COLUMNS = ["name", "branch", "y", "x", "kind", "px", "ends", "attach", "node_a", "node_b", "h", "v", "d_se", "d_sw", "length_geodesic_px",
                      "share_h", "share_v", "share_se", "share_sw", "y0", "x0", "y1", "x1"]
BRANCH_CSV_OPTIONAL = ["crack", "max_width_px", "min_width_px"]      # behind the others, each only where the branches carry the key


def crack_branches(rows, W, crack_of_label=None):
    """the ``branches`` list of ``predict_dataset`` from the host rows of ``branch_table`` (``BRANCH_COLUMNS``, and the two width columns
    where the table has them): dict(y, x, kind, px, ends, attach, nodes, links, length_geodesic_px, orientation, bbox) per branch, (y, x)
    the branch's first pixel in raster order.  ``crack_of_label`` (component label -> index into ``cracks``) adds crack; the width columns
    add max_width_px and min_width_px (``width_from_d2``)."""
    c = {k: j for j, k in enumerate(BRANCH_COLUMNS)}
    rows = np.asarray(rows, np.int64).reshape(-1, np.shape(rows)[1] if np.ndim(rows) == 2 else len(BRANCH_COLUMNS))
    nc = len(BRANCH_COLUMNS)
    # the fp64 columns for all rows at once: the arithmetic of geodesic_length and orientation_shares, element by element
    lk = rows[:, [c["h"], c["v"], c["d_se"], c["d_sw"]]]
    length = np.asarray(geodesic_length(lk[:, 0], lk[:, 1], lk[:, 2], lk[:, 3]), np.float64).reshape(-1)
    parts = lk.astype(np.float64) * np.array([1.0, 1.0, _SQRT2, _SQRT2])
    share = np.divide(parts, length[:, None], out=np.zeros_like(parts), where=length[:, None] > 0)
    wide = rows.shape[1] > nc
    width = width_from_d2(rows[:, nc:nc + 2]).tolist() if wide else None
    kinds = branch_kinds(rows)
    col = lambda *names: rows[:, [c[k] for k in names]].tolist()
    ys, xs = np.divmod(rows[:, c["label"]] - 1, W)
    # Five containers per branch, thousands per image: each batch of 700 makes the cyclic collector run, and every tenth and hundredth run
    # walks the older generations -- the whole heap of a loaded model, 60 ms measured for one such walk against 2 ms for this list.  None
    # of these objects is part of a cycle, so the collector is paused while they are built.
    paused = gc.isenabled()
    gc.disable()
    try:
        out = [dict(y=y, x=x, kind=kind, px=px, ends=end, attach=att, nodes=tuple(nodes), links=tuple(links), length_geodesic_px=n,
                    orientation=tuple(sh), bbox=tuple(box))
               for y, x, kind, (px, end, att), nodes, links, n, sh, box in zip(ys.tolist(), xs.tolist(), kinds, col("px", "end", "attach"),
                                                                                col("node_a", "node_b"), lk.tolist(), length.tolist(), share.tolist(),
                                                                                col("y0", "x0", "y1", "x1"))]
    finally:
        if paused:
            gc.enable()
    if crack_of_label is not None:
        for d, lab in zip(out, rows[:, c["crack"]].tolist()):
            d["crack"] = crack_of_label[lab]
    if wide:
        for d, (hi, lo) in zip(out, width):
            d.update(max_width_px=hi, min_width_px=lo)
    return out


def write_crack_branches(path, rows):
    """crack_branches.csv: one row per branch -- ``rows`` = (name, the image's ``branches`` list) per image; ``branch`` numbers an image's
    branches in raster order of their first pixel, ``crack`` (with ``min_crack_px``) is the numbering of crack_instances.csv"""
    first = next((b[0] for _, b in rows if b), {})
    optional = [k for k in BRANCH_CSV_OPTIONAL if k in first]
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(BRANCH_CSV_COLUMNS + optional)
        for name, branches in rows:
            for j, b in enumerate(branches):
                w.writerow([name, j, int(b["y"]), int(b["x"]), b["kind"], int(b["px"]), int(b["ends"]), int(b["attach"])] + [int(k) for k in b["nodes"]]
                           + [int(k) for k in b["links"]] + [repr(float(b["length_geodesic_px"]))] + [repr(float(k)) for k in b["orientation"]]
                           + [int(k) for k in b["bbox"]] + [int(b[k]) if k == "crack" else repr(float(b[k])) for k in optional])


def read_crack_branches(path):
    """what ``write_crack_branches`` wrote: (name, [dict]) per image that has a branch, in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    n = len(BRANCH_CSV_COLUMNS)
    optional = rows[0][n:]
    if rows[0][:n] != BRANCH_CSV_COLUMNS or optional != [k for k in BRANCH_CSV_OPTIONAL if k in optional]:
        raise ValueError(f"{path}: not a crack_branches.csv header: {rows[0]}")
    out = []
    for r in rows[1:]:
        if not out or out[-1][0] != r[0]:
            out.append((r[0], []))
        if int(r[1]) != len(out[-1][1]):
            raise ValueError(f"{path}: branch {r[1]} of {r[0]} is out of order")
        if r[4] not in BRANCH_KINDS:
            raise ValueError(f"{path}: {r[4]!r} is no branch kind")
        d = dict(y=int(r[2]), x=int(r[3]), kind=r[4], px=int(r[5]), ends=int(r[6]), attach=int(r[7]), nodes=(int(r[8]), int(r[9])),
                 links=tuple(int(v) for v in r[10:14]), length_geodesic_px=float(r[14]), orientation=tuple(float(v) for v in r[15:19]),
                 bbox=tuple(int(v) for v in r[19:23]))
        d.update({k: int(v) if k == "crack" else float(v) for k, v in zip(optional, r[n:])})
        out[-1][1].append(d)
    return out


POLYLINE_CSV_COLUMNS = ["name", "branch", "i", "y", "x", "s_px"]
POLYLINE_CSV_OPTIONAL = ["width_px"]                        # behind the others, only where the branches carry width_profile_px


def crack_polylines(branches, chain, points, widths=False):
    """adds the polyline keys of ``predict_dataset`` to the dicts of one image's ``branches`` list: ``chain`` [M] of 0 / 1 and ``points`` int
    [P_chain, 4] (``ORDER_COLUMNS``) are the host copies of ``branch_polylines``' results for the image, the chains' spans one after the
    other in the list's order.  New keys: chain (bool), points (NumPy int32 [px, 2], y then x, in order; empty for a branch that is no
    chain), start, stop, arc_px, chord_px, tortuosity, direction_deg -- the values of ``polyline_stats``, for all branches at once; a chain
    with as many inner links as pixels is a cycle (a path has px - 1) -- and with ``widths`` width_profile_px (fp64 [px], ``width_from_d2``
    of the d2 column)."""
    points = np.asarray(points, np.int64).reshape(-1, 4)
    chain = np.asarray(chain).astype(bool).reshape(-1)
    px = np.array([b["px"] for b in branches], np.int64)
    if chain.shape != px.shape:
        raise ValueError(f"{chain.size} chain flags for {px.size} branches")
    n = np.where(chain, px, 0)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(n)])
    if off[-1] != points.shape[0]:
        raise ValueError(f"{points.shape[0]} points for chains of {int(off[-1])} pixels")
    yx = points[:, :2].astype(np.int32)
    some = n > 0
    a, z = points[off[:-1][some]], points[off[1:][some] - 1]                         # the first and the last point of every chain
    arc = np.atleast_1d(arc_position(n[some] - 1, z[:, 2]))                          # the last point's diag counts the diagonal links
    dy, dx = z[:, 0] - a[:, 0], z[:, 1] - a[:, 1]
    chord = np.sqrt((dy * dy + dx * dx).astype(np.float64))
    ratio = np.divide(arc, chord, out=np.zeros_like(arc), where=chord > 0)
    width = np.atleast_1d(width_from_d2(points[:, 3])).astype(np.float64) if widths else None
    stats = iter(zip(a[:, :2].tolist(), z[:, :2].tolist(), arc.tolist(), chord.tolist(), ratio.tolist(), dy.tolist(), dx.tolist()))
    for b, c, o0, o1 in zip(branches, chain.tolist(), off[:-1].tolist(), off[1:].tolist()):
        b["chain"] = c
        if o1 > o0:
            p0, p1, s, ch, r, ddy, ddx = next(stats)
            cycle = sum(b["links"]) - b["attach"] == b["px"]
            b.update(start=tuple(p0), stop=tuple(p1), arc_px=s, chord_px=ch, tortuosity=None if ch == 0 or cycle else r,
                     direction_deg=None if ch == 0 else math.degrees(math.atan2(ddy, ddx)) % 180.0)
        else:
            b.update(start=None, stop=None, arc_px=0.0, chord_px=0.0, tortuosity=None, direction_deg=None)
        b["points"] = yx[o0:o1]
        if widths:
            b["width_profile_px"] = width[o0:o1]


def write_crack_polylines(path, rows):
    """crack_polylines.csv: one row per ordered pixel -- ``rows`` = (name, the image's ``branches`` list with the polyline keys) per image;
    ``branch`` is the numbering of crack_branches.csv, i the pixel's position along the branch, s_px its ``arc_position``, width_px (with
    ``width_radius``) its local width.  A branch that is no chain has no row."""
    first = next((b[0] for _, b in rows if b), {})
    wide = "width_profile_px" in first
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(POLYLINE_CSV_COLUMNS + (POLYLINE_CSV_OPTIONAL if wide else []))
        for name, branches in rows:
            for j, b in enumerate(branches):
                pts = np.asarray(b["points"]).reshape(-1, 2)
                s = np.atleast_1d(arc_position(np.arange(pts.shape[0]), _diag_along(pts))) if pts.shape[0] else []
                for i, (y, x) in enumerate(pts.tolist()):
                    w.writerow([name, j, i, y, x, repr(float(s[i]))] + ([repr(float(b["width_profile_px"][i]))] if wide else []))


def read_crack_polylines(path):
    """what ``write_crack_polylines`` wrote: (name, [dict(branch, points int32 [px, 2], s_px fp64 [px] and, where the file has it, width_px
    fp64 [px])]) per image that has an ordered pixel, the branches in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    n = len(POLYLINE_CSV_COLUMNS)
    if rows[0][:n] != POLYLINE_CSV_COLUMNS or rows[0][n:] not in ([], POLYLINE_CSV_OPTIONAL):
        raise ValueError(f"{path}: not a crack_polylines.csv header: {rows[0]}")
    wide = len(rows[0]) > n
    out = []
    for r in rows[1:]:
        if not out or out[-1][0] != r[0]:
            out.append((r[0], []))
        if not out[-1][1] or out[-1][1][-1]["branch"] != int(r[1]):
            if out[-1][1] and out[-1][1][-1]["branch"] > int(r[1]):
                raise ValueError(f"{path}: branch {r[1]} of {r[0]} is out of order")
            out[-1][1].append(dict(branch=int(r[1]), points=[], s_px=[], **({"width_px": []} if wide else {})))
        d = out[-1][1][-1]
        if int(r[2]) != len(d["points"]):
            raise ValueError(f"{path}: point {r[2]} of branch {r[1]} of {r[0]} is out of order")
        d["points"].append((int(r[3]), int(r[4])))
        d["s_px"].append(float(r[5]))
        if wide:
            d["width_px"].append(float(r[6]))
    for _, branches in out:
        for d in branches:
            d["points"] = np.array(d["points"], np.int32).reshape(-1, 2)
            d["s_px"] = np.array(d["s_px"], np.float64)
            if wide:
                d["width_px"] = np.array(d["width_px"], np.float64)
    return out


VERTEX_CSV_COLUMNS = ["name", "branch", "i", "index", "y", "x"]
VERTEX_CSV_OPTIONAL = ["width_px"]                          # behind the others, only where the branches carry vertex_width_px


def _closed_chain(b):
    """a chain with as many inner links as pixels: the rule of ``crack_polylines``"""
    return bool(b["chain"]) and sum(b["links"]) - b["attach"] == b["px"]


def crack_vertices(branches, points, keep, widths=False):
    """adds the keys of ``predict_dataset(simplify_px=)`` to the dicts of one image's ``branches`` list, which carry the polyline keys:
    ``points`` int [P_chain, 4] is the table ``crack_polylines`` took and ``keep`` [P_chain] of 0 / 1 the host copy of
    ``simplify_polylines``' flags for its rows.  New keys: vertices (NumPy int32 [v, 2], y then x: the kept points in order; empty for a
    branch that is no chain), vertex_index (int32 [v], their positions in ``points``), length_simplified_px (``polyline_length`` of the
    vertices, closed where the chain is -- a chain with as many inner links as pixels --, None for a branch that is no chain) and with
    ``widths`` vertex_width_px (fp64 [v], ``width_from_d2`` of the d2 column).  Returns (the image's vertices, the sum of the lengths).
    All branches at once: one pass over the image's rows, no arithmetic per branch but for the closed chains."""
    points = np.asarray(points, np.int64).reshape(-1, 4)
    keep = np.asarray(keep).reshape(-1) != 0
    n = np.array([b["points"].shape[0] for b in branches], np.int64)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(n)])
    if off[-1] != points.shape[0] or keep.shape[0] != points.shape[0]:
        raise ValueError(f"{points.shape[0]} points and {keep.shape[0]} flags for chains of {int(off[-1])} pixels")
    rows = np.nonzero(keep)[0]
    voff = np.concatenate([np.zeros(1, np.int64), np.cumsum(keep)])[off]             # the first vertex of every branch
    vc = np.diff(voff)
    verts = points[rows, :2].astype(np.int32)
    index = (rows - np.repeat(off[:-1], vc)).astype(np.int32)
    step = np.diff(verts.astype(np.float64), axis=0)
    seg = np.concatenate([np.sqrt(step[:, 0] * step[:, 0] + step[:, 1] * step[:, 1]), np.zeros(2)])      # seg[k]: from vertex k to k + 1
    ends = np.stack([voff[:-1], np.maximum(voff[1:] - 1, voff[:-1])], 1).reshape(-1)
    length = np.where(vc >= 2, np.add.reduceat(seg, ends)[::2], 0.0) if len(branches) else np.zeros(0)
    width = np.atleast_1d(width_from_d2(points[rows, 3])).astype(np.float64) if widths else None
    total = 0.0
    for b, v0, v1, s in zip(branches, voff[:-1].tolist(), voff[1:].tolist(), length.tolist()):
        b["vertices"], b["vertex_index"] = verts[v0:v1], index[v0:v1]
        if not b["chain"]:
            b["length_simplified_px"] = None
        else:
            b["length_simplified_px"] = polyline_length(verts[v0:v1], closed=True) if _closed_chain(b) else s
            total += b["length_simplified_px"]
        if widths:
            b["vertex_width_px"] = width[v0:v1]
    return int(rows.size), total


def write_crack_vertices(path, rows):
    """crack_vertices.csv: one row per vertex -- ``rows`` = (name, the image's ``branches`` list with the vertex keys) per image; ``branch``
    is the numbering of crack_branches.csv, i the vertex's position along the simplified polyline, index its position in the branch's
    ``points`` (the i of crack_polylines.csv), width_px (with ``width_radius``) its local width.  A branch that is no chain has no row."""
    first = next((b[0] for _, b in rows if b), {})
    wide = "vertex_width_px" in first
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(VERTEX_CSV_COLUMNS + (VERTEX_CSV_OPTIONAL if wide else []))
        for name, branches in rows:
            for j, b in enumerate(branches):
                for i, ((y, x), k) in enumerate(zip(np.asarray(b["vertices"]).reshape(-1, 2).tolist(), np.asarray(b["vertex_index"]).tolist())):
                    w.writerow([name, j, i, k, y, x] + ([repr(float(b["vertex_width_px"][i]))] if wide else []))


def read_crack_vertices(path):
    """what ``write_crack_vertices`` wrote: (name, [dict(branch, vertices int32 [v, 2], vertex_index int32 [v] and, where the file has it,
    width_px fp64 [v])]) per image that has a vertex, the branches in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    n = len(VERTEX_CSV_COLUMNS)
    if rows[0][:n] != VERTEX_CSV_COLUMNS or rows[0][n:] not in ([], VERTEX_CSV_OPTIONAL):
        raise ValueError(f"{path}: not a crack_vertices.csv header: {rows[0]}")
    wide = len(rows[0]) > n
    out = []
    for r in rows[1:]:
        if not out or out[-1][0] != r[0]:
            out.append((r[0], []))
        if not out[-1][1] or out[-1][1][-1]["branch"] != int(r[1]):
            if out[-1][1] and out[-1][1][-1]["branch"] > int(r[1]):
                raise ValueError(f"{path}: branch {r[1]} of {r[0]} is out of order")
            out[-1][1].append(dict(branch=int(r[1]), vertices=[], vertex_index=[], **({"width_px": []} if wide else {})))
        d = out[-1][1][-1]
        if int(r[2]) != len(d["vertices"]):
            raise ValueError(f"{path}: vertex {r[2]} of branch {r[1]} of {r[0]} is out of order")
        d["vertex_index"].append(int(r[3]))
        d["vertices"].append((int(r[4]), int(r[5])))
        if wide:
            d["width_px"].append(float(r[6]))
    for _, branches in out:
        for d in branches:
            d["vertices"] = np.array(d["vertices"], np.int32).reshape(-1, 2)
            d["vertex_index"] = np.array(d["vertex_index"], np.int32)
            if wide:
                d["width_px"] = np.array(d["width_px"], np.float64)
    return out


def crack_geojson(rows):
    """the FeatureCollection of crack_polylines.geojson as a dict: one Feature per chain of ``rows`` = (name, the image's ``branches`` list
    with the vertex keys) per image.  The geometry is a LineString of [x, y] in pixels -- a closed chain repeats its first vertex -- or, for
    a chain of one vertex, a Point; the properties are name, branch (the numbering of crack_branches.csv), kind, closed, px, n_vertices,
    arc_px, length_simplified_px and, where the dicts have them, crack, max_width_px and min_width_px."""
    features = []
    for name, branches in rows:
        for j, b in enumerate(branches):
            if not b["chain"]:
                continue
            xy = [[int(x), int(y)] for y, x in np.asarray(b["vertices"]).reshape(-1, 2).tolist()]
            closed = _closed_chain(b)
            if len(xy) == 1:
                geometry = {"type": "Point", "coordinates": xy[0]}
            else:
                geometry = {"type": "LineString", "coordinates": xy + (xy[:1] if closed else [])}
            prop = dict(name=name, branch=j, kind=b["kind"], closed=closed, px=int(b["px"]), n_vertices=len(xy), arc_px=float(b["arc_px"]),
                        length_simplified_px=float(b["length_simplified_px"]))
            prop.update({k: int(b[k]) if k == "crack" else float(b[k]) for k in ("crack", "max_width_px", "min_width_px") if k in b})
            features.append({"type": "Feature", "geometry": geometry, "properties": prop})
    return {"type": "FeatureCollection", "features": features}


def write_crack_geojson(path, rows):
    """crack_polylines.geojson: ``crack_geojson`` of ``rows`` with sorted keys, so that two runs give the same bytes"""
    with open(path, "w") as fh:
        fh.write(json.dumps(crack_geojson(rows), sort_keys=True))
        fh.write("\n")


GAP_CSV_COLUMNS = ["name", "gap", "y", "x", "to_y", "to_x", "gap_px", "d2", "kind", "mutual"]
GAP_CSV_OPTIONAL = ["crack", "to_crack"]                    # behind the others, where the gaps carry them (``min_crack_px``)
GAP_KINDS = ("end_end", "end_side")


def crack_gaps(rows, W, crack_of_label=None):
    """the ``gaps`` list of ``predict_dataset`` from the host rows of ``gap_table`` (``GAP_COLUMNS``) of one image: dict(y, x, to, gap_px, d2,
    kind, mutual) per gap, in raster order of the source (y, x); ``to`` = (y, x) of the target, kind "end_end" where the target is an end
    or an isolated pixel, else "end_side".  ``crack_of_label`` (component label -> index into ``cracks``) adds crack and to_crack."""
    c = {k: j for j, k in enumerate(GAP_COLUMNS)}
    rows = np.asarray(rows, np.int64).reshape(-1, len(GAP_COLUMNS))
    py, px = np.divmod(rows[:, c["p"]], W)
    qy, qx = np.divmod(rows[:, c["q"]], W)
    ends = (rows[:, c["class_q"]] == TOPO_ISOLATED) | (rows[:, c["class_q"]] == TOPO_END)
    length = np.asarray(gap_length(rows[:, c["d2"]]), np.float64).reshape(-1)
    out = [dict(y=y, x=x, to=(ty, tx), gap_px=g, d2=d2, kind=GAP_KINDS[0] if e else GAP_KINDS[1], mutual=bool(m))
           for y, x, ty, tx, g, d2, e, m in zip(py.tolist(), px.tolist(), qy.tolist(), qx.tolist(), length.tolist(), rows[:, c["d2"]].tolist(),
                                                ends.tolist(), rows[:, c["mutual"]].tolist())]
    if crack_of_label is not None:
        for d, (a, b) in zip(out, rows[:, [c["label_p"], c["label_q"]]].tolist()):
            d.update(crack=crack_of_label[a], to_crack=crack_of_label[b])
    return out


def write_crack_gaps(path, rows):
    """crack_gaps.csv: one row per gap -- ``rows`` = (name, the image's ``gaps`` list) per image; ``gap`` numbers an image's gaps in raster
    order of their source, ``crack`` / ``to_crack`` (with ``min_crack_px``) are the numbering of crack_instances.csv"""
    first = next((g[0] for _, g in rows if g), {})
    optional = [k for k in GAP_CSV_OPTIONAL if k in first]
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(GAP_CSV_COLUMNS + optional)
        for name, gaps in rows:
            for j, g in enumerate(gaps):
                w.writerow([name, j, int(g["y"]), int(g["x"]), int(g["to"][0]), int(g["to"][1]), repr(float(g["gap_px"])), int(g["d2"]), g["kind"],
                            int(bool(g["mutual"]))] + [int(g[k]) for k in optional])


def read_crack_gaps(path):
    """what ``write_crack_gaps`` wrote: (name, [dict]) per image that has a gap, in the file's order"""
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    n = len(GAP_CSV_COLUMNS)
    optional = rows[0][n:]
    if rows[0][:n] != GAP_CSV_COLUMNS or optional not in ([], GAP_CSV_OPTIONAL):
        raise ValueError(f"{path}: not a crack_gaps.csv header: {rows[0]}")
    out = []
    for r in rows[1:]:
        if not out or out[-1][0] != r[0]:
            out.append((r[0], []))
        if int(r[1]) != len(out[-1][1]):
            raise ValueError(f"{path}: gap {r[1]} of {r[0]} is out of order")
        if r[8] not in GAP_KINDS or r[9] not in ("0", "1"):
            raise ValueError(f"{path}: {r[8]!r}, {r[9]!r} is no gap kind and mutual flag")
        d = dict(y=int(r[2]), x=int(r[3]), to=(int(r[4]), int(r[5])), gap_px=float(r[6]), d2=int(r[7]), kind=r[8], mutual=r[9] == "1")
        d.update({k: int(v) for k, v in zip(optional, r[n:])})
        out[-1][1].append(d)
    return out


class _Saver:
    """The files ``test.py --sf_save_image`` writes (model/utils/save_output.py), fed with uint8 buffers through a ring of pinned slots:
    ``push`` enqueues non-blocking copies on the current stream and records the slot's event, ``drain`` waits on that event alone and
    encodes with PIL -- the caller drains batch k after it has enqueued batch k + 1.

    A batch is (img [B,H,W,3], raw [B,H,W,1], planes [B,S,H,W], kern [B * nP,1,K,K]) of equal images, or, with ``layout`` = one
    (pixel offset, H, W, first kernel, kernels) per image, flat pools of images of any size: img [3 * npix] interleaved per image, raw [npix],
    planes [1,S,npix], kern [sum of kernels,1,K,K].  With ``skeletons`` a fifth tensor follows, skel [npix] of 0 / 255 laid out like raw, and
    goes to skeletons/<name>; with ``bridged`` a sixth of the same kind, which goes to skeletons_bridged/<name>."""

    def __init__(self, save_dir, thresholds, skeletons=False, bridged=False):
        self.dir = save_dir
        self.th_names = [f"th_{thresholds[i]:.2f}" for i in SAVE_THRESHOLD_IDX if i < len(thresholds)] + ["th_-1.00"]
        for d in ["images", "kernels", "kernels_origin"] + [os.path.join("masks", t) for t in self.th_names] + ["skeletons"] * bool(skeletons) + ["skeletons_bridged"] * bool(bridged):
            os.makedirs(os.path.join(save_dir, d), exist_ok=True)
        self.ring, self.n, self.pending = [None] * _SLOTS, 0, []

    def push(self, fnames, tensors, layout=None):
        """tensors: device tensors of any dtype; their bytes go back to back into the slot's pinned buffer."""
        need = sum(-(-t.numel() * t.element_size() // 16) * 16 for t in tensors)          # every view starts at a multiple of 16
        slot = self.ring[self.n % _SLOTS]
        if slot is None or slot[0].numel() < need:
            slot = self.ring[self.n % _SLOTS] = (torch.empty(need, dtype=torch.uint8).pin_memory(), torch.cuda.Event())
        self.n += 1
        host, ev = slot
        views, off = [], 0
        for t in tensors:
            nb = t.numel() * t.element_size()
            v = host[off:off + nb].view(t.dtype).view(t.shape)
            v.copy_(t, non_blocking=True)
            views.append(v)
            off += -(-nb // 16) * 16
        ev.record(torch.cuda.current_stream(tensors[0].device))
        self.pending.append((fnames, views, ev, layout))

    def drain(self, keep=0):
        from PIL import Image
        while len(self.pending) > keep:
            fnames, views, ev, layout = self.pending.pop(0)
            img, raw, planes, kern = views[:4]
            ev.synchronize()                                 # this slot's copies only
            img, raw, planes = img.numpy(), raw.numpy(), planes.numpy()
            skel = views[4].numpy() if len(views) > 4 else None
            bridged = views[5].numpy() if len(views) > 5 else None
            nP = kern.shape[0] // len(fnames)
            for b, name in enumerate(fnames):
                if layout is None:
                    img_b, raw_b, planes_b, k0 = img[b], raw[b, :, :, 0], planes[b], b * nP
                else:
                    o, H, W, k0, nP = layout[b]
                    img_b, raw_b = img[3 * o:3 * (o + H * W)].reshape(H, W, 3), raw[o:o + H * W].reshape(H, W)
                    planes_b = planes[0, :, o:o + H * W].reshape(-1, H, W)
                Image.fromarray(img_b).save(os.path.join(self.dir, "images", name))
                for j, t in enumerate(self.th_names[:-1]):
                    Image.fromarray(planes_b[j]).save(os.path.join(self.dir, "masks", t, name))
                Image.fromarray(raw_b).save(os.path.join(self.dir, "masks", "th_-1.00", name))
                if skel is not None:
                    o, H, W = layout[b][:3]
                    Image.fromarray(skel[o:o + H * W].reshape(H, W)).save(os.path.join(self.dir, "skeletons", name))
                if bridged is not None:
                    o, H, W = layout[b][:3]
                    Image.fromarray(bridged[o:o + H * W].reshape(H, W)).save(os.path.join(self.dir, "skeletons_bridged", name))
                stem = name.replace(".png", "")
                for j in range(nP):                          # save_kernel: 441 values per patch, on the host
                    k = kern[k0 + j]
                    for sub, tail, q in (("kernels", "", k / torch.max(k)), ("kernels_origin", "_origin", k / torch.sum(k))):
                        q8 = torch.nan_to_num(q, nan=0.0).mul(255).byte().numpy()[0]
                        Image.fromarray(q8).save(os.path.join(self.dir, sub, f"{stem}_{j}{tail}.png"))


@torch.no_grad()
def evaluate_dataset(model, loader, *, ksize=21, thresholds=THRESHOLDS, surface_distance=False, classification=False, save_dir=None,
                     pr_tolerance=None, cldice_threshold=None):
    """``inference_for_ss`` (model/engine/inference.py:25-207) over a ``DeviceTestLoader``: per batch the computation of ``evaluate_batch``
    -- with the stitch, the clip and the 8-bit quantisation in one kernel (csbsr_stitch_clip_u8) instead of JointPatch's copy and two masked
    assignments -- accumulated into the reference's final report.  ``model`` is any callable with JointModel's evaluation signature.

    Returns dict(fnames, psnr [N], ssim [N], kernel_psnr [N * nPatch], iou [N, T] (fp32, as evaluate_batch returns them), summary);
    ``surface_distance`` adds hd, msd [N, T] float64 and the counters hd_outliers, msd_outliers summed over the batches;
    ``classification`` adds acc, sens, spec [N] float64 at threshold index 49 (integer counts on the device, one fp64 division on the
    host).  ``summary`` is ``summarize`` of those arrays.  ``pr_tolerance`` = a radius in pixels adds pr_counts [N, 4, T] int64 -- per image
    and threshold (n_pred, tp_pred, tp_gt, n_gt) of ``pr_sweep``: a predicted pixel counts when a ground-truth pixel lies within the
    radius, and the other way round -- and the keys of ``summarize_pr`` (ODS, ODS_threshold, OIS, AP, P_at_ODS, R_at_ODS) to ``summary``;
    None (the default) adds nothing.  ``cldice_threshold`` = a float strictly inside (0, 1) adds cl_counts [N, 4] int64 -- per image
    (|S_P|, |S_P & V_L|, |S_L|, |S_L & V_P|) of ``centerline_counts``, S the Guo-Hall skeletons of the map binarised at that threshold and of
    the mask -- and the keys of ``summarize_cldice`` (clDice, Tprec, Tsens, clDice_pooled) to ``summary``; None (the default) adds nothing.
    It is ONE threshold, not the sweep: the binary maps of the 99 thresholds are nested, their skeletons are not, so a sweep would be 99
    thinnings per image.

    ``save_dir`` writes what ``test.py --sf_save_image`` writes: images/<fname>, masks/th_<t:.2f>/<fname> for the threshold indices
    [0, 9, 19, ..., 89, 98], masks/th_-1.00/<fname> for the raw map, kernels/<stem>_<j>.png, kernels_origin/<stem>_<j>_origin.png, and
    iou_log.csv (and, with ``pr_tolerance``, pr_log.csv next to it: ``write_pr_log``; with ``cldice_threshold``, cldice_log.csv:
    ``write_cldice_log``).  Images and masks leave the device as uint8
    (csbsr_stitch_clip_u8, csbsr_threshold_planes_u8) through pinned slots with non-blocking copies; PIL encodes batch k while the device runs batch k + 1, and the host waits on a slot's event only.  Without
    ``save_dir`` the metrics stay on the device until the last batch has been enqueued (the surface distances, whose second half is host
    work, excepted)."""
    th32 = torch.tensor([float(t) for t in thresholds], dtype=torch.float32)
    if classification and len(thresholds) <= CLASSIFICATION_IDX:
        raise ValueError(f"classification metrics are taken at threshold index {CLASSIFICATION_IDX}: {len(thresholds)} thresholds given")
    if pr_tolerance is not None:
        pr_tol2(pr_tolerance)                                # a bad radius is refused before anything runs
    if cldice_threshold is not None:
        cldice_threshold = unit_threshold(cldice_threshold, "cldice_threshold")
    saver = _Saver(save_dir, thresholds) if save_dir is not None else None
    save_th = None
    fnames, acc = [], {k: [] for k in ("psnr", "ssim", "kernel_psnr", "iou", "counts", "hd", "msd", "pr", "cl")}
    hd_out = msd_out = 0
    for imgs, sr_targets, masks, kernel_targets, names, img_shape, seg_shape in loader:
        fnames += list(names)
        imgs = imgs.view(-1, *imgs.shape[2:])
        kernel_targets = kernel_targets.view(-1, 1, *kernel_targets.shape[2:])
        dummy = torch.zeros((imgs.shape[0], 1, ksize, ksize))
        sr_p, seg_p, kernel_preds = model(imgs, dummy, sr_targets=sr_targets)
        sr_preds, sr_u8 = stitch_clip_u8(sr_p, img_shape, clip=True, want_u8=saver is not None)
        segment_preds, seg_u8 = stitch_clip_u8(seg_p, seg_shape, clip=False, want_u8=saver is not None)
        kernel_preds = kernel_preds.clamp(0, 1)
        ps, ss = psnr_ssim(sr_preds, sr_targets)
        kps, _ = psnr_ssim(_kernel_for_psnr(model, kernel_preds, kernel_targets), kernel_targets)
        acc["psnr"].append(ps)
        acc["ssim"].append(ss)
        acc["kernel_psnr"].append(kps)
        acc["iou"].append(iou_sweep(segment_preds, masks, thresholds))
        if classification:
            acc["counts"].append(classification_counts(segment_preds, masks, th32[CLASSIFICATION_IDX].to(segment_preds.device)))
        if pr_tolerance is not None:
            acc["pr"].append(pr_sweep(segment_preds, masks, thresholds, pr_tolerance))
        if cldice_threshold is not None:
            acc["cl"].append(centerline_counts(segment_preds, masks, cldice_threshold))
        if saver is not None:
            if save_th is None:
                save_th = th32[[i for i in SAVE_THRESHOLD_IDX if i < len(thresholds)]].to(segment_preds.device)
            planes = threshold_planes_u8(segment_preds[:, 0], save_th)
            saver.push(list(names), [sr_u8, seg_u8, planes, kernel_preds.to(torch.float32)])
            saver.drain(keep=1)                              # encode the batch before this one while the device runs this one
        if surface_distance:
            sd = surface_distance_sweep(segment_preds, masks, thresholds)
            acc["hd"].append(sd["hd"])
            acc["msd"].append(sd["msd"])
            hd_out += sd["hd_outliers"]
            msd_out += sd["msd_outliers"]
    if not fnames:
        raise ValueError("the test set is empty")
    if saver is not None:
        saver.drain()
    out = {"fnames": fnames}
    for k in ("psnr", "ssim", "kernel_psnr", "iou"):
        out[k] = torch.cat(acc[k]).cpu().numpy()
    if surface_distance:
        out.update(hd=np.concatenate(acc["hd"]), msd=np.concatenate(acc["msd"]), hd_outliers=int(hd_out), msd_outliers=int(msd_out))
    if classification:
        out["acc"], out["sens"], out["spec"] = classification_scores(torch.cat(acc["counts"]).cpu().numpy())
    out["summary"] = summarize(out["psnr"], out["ssim"], out["kernel_psnr"], out["iou"], out.get("hd"), out.get("msd"))
    if pr_tolerance is not None:
        out["pr_counts"] = torch.cat(acc["pr"]).cpu().numpy().astype(np.int64)
        out["summary"].update(summarize_pr(out["pr_counts"], thresholds))
    if cldice_threshold is not None:
        out["cl_counts"] = torch.cat(acc["cl"]).cpu().numpy().astype(np.int64)
        out["summary"].update(summarize_cldice(out["cl_counts"]))
    if save_dir is not None:
        write_iou_log(os.path.join(save_dir, "iou_log.csv"), out["iou"], thresholds, fnames)
        if pr_tolerance is not None:
            write_pr_log(os.path.join(save_dir, "pr_log.csv"), out["pr_counts"], thresholds, fnames)
        if cldice_threshold is not None:
            write_cldice_log(os.path.join(save_dir, "cldice_log.csv"), out["cl_counts"], fnames)
    return out


# ------------------------------------------------------------------------------------------------ prediction without ground truth
def _hist_and_widest(d2, hist):
    """one image's histogram with one more int64 behind it: max over the pixels of  d2 * H W + (H W - 1 - index) , whose maximum is the first
    pixel in raster order with the largest d2 (< H W when d2 is 0 everywhere) -- a single integer reduction, nothing read by the host"""
    hw = d2.numel()
    key = d2.view(-1).to(torch.int64) * hw + torch.arange(hw - 1, -1, -1, dtype=torch.int64, device=d2.device)
    return torch.cat([hist.view(-1).to(torch.int64), key.max().view(1)])


def _topology_ints(sk):
    """(topo, the image's twelve integers as one int64 device tensor -- the ten counts, the skeleton's 8-connected components and the
    junction clusters --, the junction labels) of one skeleton plane [1, H, W]: nothing is read by the host"""
    topo, counts = skeleton_topology(sk)
    jl = _junction_labels(topo)
    ints = torch.cat([counts.view(-1).to(torch.int64), _count_roots(label_components(sk.to(torch.float32), 0.5)), _count_roots(jl)])
    return topo, ints, jl


def _order_into(bl, topo, d2, rmaps, btables, ptables, simplify_px=None, ktables=None):
    """the polylines of one image's branch labels: its rank map, the chain flag behind the image's branch rows, its ordered points and,
    with ``simplify_px``, the kept flag of every point"""
    H, W = bl.shape[-2:]
    rank, diag = order_branches(bl, topo)
    chain, offsets, points = branch_polylines(bl, rank, diag, d2)
    if simplify_px is not None:
        ktables.append(simplify_polylines(offsets, points, simplify_px)[0])
    rmaps.append(rank.view(H, W))
    btables[-1] = torch.cat([btables[-1], chain.to(torch.int32).view(-1, 1)], 1)
    ptables.append(points)


def _bridge_into(j, topo, lab, sk, gap, to, px, gtables, gmaps, glabels, bridged_u8, count_cracks):
    """the gaps of one image: its gap rows, bridge map, group labels and bridged skeleton (0 / 255), and two integers in front of the
    topology's twelve in the image's row of the unit's read -- bridge_px = |bridges & ~skeleton| and, with ``count_cracks``, the labels that
    have a skeleton pixel (else 0)"""
    _, H, W = topo.shape
    lab = lab.view(1, H, W)
    gq, gd2 = endpoint_gaps(topo, lab, gap, to)
    rows = gap_table(topo, lab, gq, gd2)
    rows[:, 0] = j                                           # the image within the unit
    gtables.append(rows)
    bm = draw_bridges(gq).view(-1)
    gmaps.append(bm.view(H, W))
    glabels.append(gap_groups(lab, gq).view(H, W))
    bridged_u8.copy_((sk | bm) * 255)
    if count_cracks:
        seen = torch.zeros(H * W + 1, dtype=torch.bool, device=lab.device)
        seen[(lab.view(-1) * (sk != 0)).long()] = True
        n_seen = seen[1:].sum()
    else:
        n_seen = torch.zeros((), dtype=torch.int64, device=lab.device)
    ints = torch.stack([(bm * (sk == 0)).sum(), n_seen])
    k = TOPO_COUNTS + 2
    px[-1] = torch.cat([px[-1][:-k], ints, px[-1][-k:]])


@torch.no_grad()
def predict_dataset(model, loader, *, ksize=21, thresholds=THRESHOLDS, save_dir=None, measure_threshold=None, min_crack_px=None,
                    width_radius=None, topology=False, prune_spur_px=None, branches=False, polylines=False, simplify_px=None, bridge_gap_px=None,
                    bridge_to="any"):
    """``inference_tti_building`` (model/engine/inference.py:210-273) over a ``DevicePredictLoader``: LR images only, every window through
    ``model`` (any callable with JointModel's evaluation signature), and the owned part of every output patch into its image by
    csbsr_stitch_tiles_u8 -- the SR image clipped, as bytes; the map unclipped, as fp32 and as bytes.  Unlike the reference's unfold, every
    input pixel gets an output, and with the loader's ``halo`` every tile is convolved with real context instead of zero padding.

    A GENERATOR: per image, in the set's order, it yields dict(name, sr_u8 [H,W,3] uint8, map_u8 [H,W] uint8, map_f32 [H,W] fp32,
    kernels [tiles,1,K,K] fp32 clamped to [0, 1]) -- device tensors, views of the pools of the image's work unit.  The pools of one unit
    are allocated when the unit starts and belong to whoever keeps the yielded tensors; the driver itself holds one unit at a time.

    ``save_dir`` writes what ``evaluate_dataset`` writes, minus iou_log.csv -- images/<name>, masks/th_<t:.2f>/<name> for the threshold
    indices [0, 9, 19, ..., 89, 98] (one csbsr_threshold_planes_u8 launch over the unit's flat map pool), masks/th_-1.00/<name>,
    kernels/<stem>_<j>.png and kernels_origin/<stem>_<j>_origin.png, j over the image's tiles -- through the same ring of pinned slots; the
    files of the last units are complete when the generator is exhausted.

    ``measure_threshold`` = a float strictly inside (0, 1) adds three keys to every yielded dict: crack_px (int), the pixels with
    map_f32 - t > 0; skeleton_px (int), the size of that region's Guo-Hall skeleton (``skeletonize``) -- the crack's length in pixels --;
    mean_width_px = crack_px / skeleton_px in fp64 (0.0 for an empty skeleton).  The skeleton is taken on the stitched map of the whole
    image, never per tile, and the two integers of all the images of a work unit come back in one read.  With ``save_dir`` it also writes
    skeletons/<name> (0 / 255) through the ring and, when the generator is exhausted, crack_stats.csv.  None (the default) adds nothing.

    ``min_crack_px`` = k, a whole number >= 1 (it needs ``measure_threshold``; anything else is a ValueError before the model runs), measures
    crack by crack.  With R the region map_f32 - t > 0 and K the pixels of R's 8-connected components of at least k pixels
    (``label_components``, ``keep_components``): crack_px = |K|; the skeleton is skeletonize(R) & K -- one thinning: two components never
    share a 3 x 3 neighbourhood, so it is the skeleton of K --; skeleton_px and mean_width_px are taken over K.  New keys: removed_px =
    |R| - |K|; n_cracks; labels, device int32 [H, W] with the removed components 0; cracks, a list in raster order of the first pixel of
    dict(y, x, area_px, length_px, mean_width_px, bbox=(y0, x0, y1, x1)) -- (y, x) the first pixel, length_px the crack's skeleton pixels, the
    box inclusive (``crack_instances``).  The integers of a unit still come back in one read, the unit's tables in one more.  With
    ``save_dir``, skeletons/<name> shows the kept skeleton, crack_stats.csv holds the values over K, and crack_instances.csv
    (``write_crack_instances``) is written when the generator is exhausted.  None (the default) adds nothing.

    ``width_radius`` = r, a whole number 1 .. 128 (it needs ``measure_threshold`` too; anything else is a ValueError before the model runs),
    takes the local width (``skeleton_width``) at the pixels of the skeleton the call reports -- with ``min_crack_px`` the kept
    skeleton -- always against the region R of the whole stitched map: for a pixel of a kept component the nearest pixel outside K is never
    closer than the nearest background pixel, so the distances against R are the distances against K.  New keys: max_width_px,
    median_width_px, p95_width_px, centerline_width_px (floats, ``summarize_width_hist``; lower bounds where saturated_px > 0), saturated_px
    (int), widest = (y, x) of the first centerline pixel in raster order with the largest d2 (None for an empty skeleton), width_hist (NumPy
    int64 [r^2 + 2]) and width_d2 (device int32 [H, W]).  mean_width_px keeps its meaning, area over length.  With ``min_crack_px`` every dict
    of ``cracks`` gains max_width_px and widest.  One more read per unit (the stacked histograms); the per-crack columns travel with the
    unit's tables.  With ``save_dir``, crack_widths.csv (``write_crack_widths``) and, with ``min_crack_px``, crack_instance_widths.csv
    (``write_crack_instance_widths``) are written when the generator is exhausted.  None (the default) adds nothing.

    ``topology`` = True (only True and False are accepted, and True needs ``measure_threshold``; anything else is a ValueError before the
    model runs) describes the shape of the skeleton the call reports -- with ``min_crack_px`` the kept skeleton -- (DESIGN 1.13,
    ``skeleton_topology``).  New keys: endpoints, junction_px, isolated_px (pixels of that class), junctions (the 8-connected clusters of
    junction pixels), loops (the enclosed cells: the skeleton's 8-connected components minus its Euler number), links = (h, v, d_se, d_sw),
    length_geodesic_px (``geodesic_length``: reads long by up to 8.24 % on a straight line that is neither axis-parallel nor at 45 degrees),
    orientation (``orientation_shares``), mean_width_geodesic_px = crack_px / length_geodesic_px (0.0 for a length of 0) and topology_map
    (device uint8 [H, W], the topo bytes).  skeleton_px, length_px and mean_width_px keep their meaning.  With ``min_crack_px`` every dict of
    ``cracks`` gains endpoints, junctions, loops, links, length_geodesic_px and orientation (``crack_topology``).  The integers travel in the
    unit's one read, the per-crack columns with the unit's tables.  With ``save_dir``, crack_topology.csv (``write_crack_topology``) and,
    with ``min_crack_px``, crack_instance_topology.csv (``write_crack_instance_topology``) are written when the generator is exhausted.
    False (the default) adds nothing: no key, no file, no launch.

    ``prune_spur_px`` = L, a whole number 1 .. 64 (it needs ``measure_threshold``; anything else is a ValueError before the model runs),
    removes the centerline's side branches of up to L pixels before anything is measured on it (``prune_spurs``): the skeleton
    the call reports is prune(skeletonize(R)), with ``min_crack_px`` prune(skeletonize(R)) & K -- one pruning: the skeletons of two
    components of R are never 8-adjacent, so it is the pruning of the kept skeleton.  skeleton_px and mean_width_px, every crack's
    length_px and mean_width_px, every ``width_radius`` and ``topology`` result and skeletons/<name> describe the pruned skeleton.  New
    key: spur_px (int), the centerline pixels removed (over K with ``min_crack_px``), so that skeleton_px + spur_px is the call's
    skeleton_px without the option; with ``min_crack_px`` every dict of ``cracks`` gains spur_px too.  A branch of up to L pixels that hangs
    off a loop or a longer structure goes even where it is a real crack, and of two unequal arms at a crack's end the shorter goes when it
    is at most L long.  The integers travel in the unit's one read, the per-crack column with the unit's tables.  With ``save_dir``,
    crack_spurs.csv (``write_crack_spurs``) and, with ``min_crack_px``, crack_instance_spurs.csv (``write_crack_instance_spurs``) are
    written when the generator is exhausted; crack_stats.csv and every other file keep their columns.  None (the default) adds nothing: no
    key, no file, no launch.

    ``branches`` = True (only True and False are accepted, and True needs ``topology`` = True; anything else is a ValueError before the
    model runs) adds the branch table (``label_branches``, ``branch_table``) of the skeleton the call reports -- pruned with
    ``prune_spur_px``, kept with ``min_crack_px`` --: one row per centerline segment between junctions.  New keys: n_branches; branch_kinds
    (a dict over ``BRANCH_KINDS`` of counts); longest_branch_px (the largest length_geodesic_px of a branch that is not isolated, as in
    ``summarize_branches``); branch_map (device int32 [H, W], the branch
    labels); branches, a list in raster order of the first pixel of dict(y, x, kind, px, ends, attach, nodes=(a, b), links,
    length_geodesic_px, orientation, bbox) (``crack_branches``) -- with ``min_crack_px`` each also carries crack, the index into ``cracks``,
    and every dict of ``cracks`` gains n_branches; with ``width_radius`` each carries max_width_px and min_width_px.  A branch that
    touches three or more junction clusters names only the smallest and the largest in nodes, and its attach exceeds 2.  The branch rows
    travel in a tensor of their own, one more read per unit.  With ``save_dir``, crack_branches.csv (``write_crack_branches``) is written
    when the generator is exhausted; no other file gains a column.  False (the default) adds nothing: no key, no file, no launch.

    ``polylines`` = True (only True and False are accepted, and True needs ``branches`` = True; anything else is a ValueError before the
    model runs) orders the pixels of every branch from end to end (``order_branches``, ``branch_polylines``), on the skeleton
    the call reports, as ``branches`` does.  New keys: n_chains (the branches that are ordered); unordered_branch_px (the pixels of the
    others: a branch through a full 2 x 2 quad is no chain and is not ordered); rank_map (device int32 [H, W], the position of every pixel
    along its branch, -1 where there is none).  Every dict of ``branches`` gains chain; start and stop, (y, x) -- a path starts at its end
    with the smaller linear index, a closed chain at its first pixel in raster order --; arc_px, the chain-code length of the inner links between
    them (it counts inner links only: length_geodesic_px also counts the attach links out to the junction centres); chord_px; tortuosity
    = arc_px / chord_px (None for a zero chord and for a closed chain); direction_deg in [0, 180) (None for a zero chord) (``polyline_stats``);
    points, NumPy int32 [px, 2], y then x, in order (empty for a branch that is no chain); and with ``width_radius`` width_profile_px, fp64
    [px], ``width_from_d2`` at the points.  The points of a unit travel in one tensor, one more read per unit; the chain flags travel with
    the branch rows.  With ``save_dir``, crack_polylines.csv (``write_crack_polylines``) is written when the generator is exhausted; no
    other file gains a column.  False (the default) adds nothing: no key, no file, no launch.

    ``simplify_px`` = T, a multiple of 0.25 in [0, 16] (``simplify_tolerance``; it needs ``polylines`` = True; anything else is a ValueError
    before the model runs), simplifies the polylines the call reports -- kept with ``min_crack_px``, pruned with ``prune_spur_px`` -- by
    Douglas-Peucker with the tolerance T in pixels (``simplify_polylines``): a point stays where dropping it would move the line
    by more than T.  New keys: n_vertices (int) and length_simplified_px (the sum over the chains).  Every dict of ``branches`` gains
    vertices, NumPy int32 [v, 2], y then x (empty for a branch that is no chain); vertex_index, int32 [v], their positions in points;
    length_simplified_px, the Euclidean length of the simplified polyline (``polyline_length``; with the closing segment for a closed
    chain, None for a branch that is no chain) -- exact on a digital straight line once T exceeds the rounding of the line's ends, 1 px at
    the most, where arc_px reads up to 8.24 % long --; and with
    ``width_radius`` vertex_width_px, fp64 [v].  The kept flags of a unit travel in one tensor, one more read per unit.  With ``save_dir``,
    crack_vertices.csv (``write_crack_vertices``) and crack_polylines.geojson (``write_crack_geojson``) are written when the generator is
    exhausted; no other file gains a column.  None (the default) adds nothing: no key, no file, no launch.

    ``bridge_gap_px`` = G, a whole number 2 .. 64 (``gap_radius``; it needs ``measure_threshold`` and ``topology`` = True), with ``bridge_to``
    = "any" (the default) or "end" (anything else, or a ``bridge_to`` other than "any" without ``bridge_gap_px``, is a ValueError before the
    model runs), says which of the cracks the call reports are one crack (``endpoint_gaps``): a map thresholded at one level
    breaks a thin crack wherever it dips below the threshold.  For every end and isolated pixel of the skeleton the call reports -- pruned
    with ``prune_spur_px``, kept with ``min_crack_px`` -- it finds the nearest centerline pixel of ANOTHER crack within G pixels ("end": the
    nearest end or isolated pixel), the first in raster order among equals: the end's gap.  The cracks are those of ``cracks``: the labels
    are the kept labels with ``min_crack_px``, else ``label_components`` of the stitched map at ``measure_threshold``.  New keys: n_gaps;
    n_mutual_gaps (the gaps whose target's gap leads back: a mutual pair is two of them); gap_length_px (the sum of the gaps' lengths, a
    mutual pair counted once) and max_gap_px (``summarize_gaps``); bridge_px, the pixels of the bridges -- the 8-connected Bresenham line
    of every gap, ``draw_bridges`` -- that are no skeleton pixels; n_cracks_bridged, the number of groups when the cracks a gap joins count
    as one: with ``min_crack_px`` n_cracks minus the joins, the groups among the dicts of ``cracks``; without it the components of R that
    have a pixel on the reported skeleton (the number to compare it with) minus the joins; gaps, a list in raster order of the source of
    dict(y, x, to=(y, x), gap_px, d2, kind, mutual) -- kind "end_end" where the target is an end or an isolated pixel, else "end_side"
    (``crack_gaps``) --, with ``min_crack_px`` each also with crack and to_crack, indices into ``cracks``; bridge_map (device uint8 [H, W],
    0 / 1) and bridged_labels (device int32 [H, W]: every pixel of a crack carries the smallest label of its group, ``gap_groups``).  With
    ``min_crack_px`` every dict of ``cracks`` gains group, the index into ``cracks`` of its group's first crack, and gaps, the number of gaps
    that start in it.  The bridged skeleton is NOT re-measured: topology, branches, polylines and widths describe the unbridged one.  There
    is no direction test: an end bridges to the nearest other crack even when that crack runs beside it -- ``bridge_to`` = "end" and kind /
    mutual are the filters offered.  A fragment below ``min_crack_px`` is removed before the bridging and cannot be rescued by it, and a
    bridge may run over pixels of the end's own crack.  The unit's integers stay in its one read; the gap rows travel in a tensor of
    their own, one more read per unit.  With ``save_dir``, skeletons_bridged/<name> (0 / 255, skeleton | bridges) goes through the ring and
    crack_gaps.csv (``write_crack_gaps``) is written when the generator is exhausted; no other file gains a column.  None (the default)
    adds nothing: no key, no file, no launch."""
    if topology is not True and topology is not False:
        raise ValueError(f"topology is True or False, got {topology!r}")
    if topology and measure_threshold is None:
        raise ValueError("topology describes the skeleton of measure_threshold: give measure_threshold too")
    if branches is not True and branches is not False:
        raise ValueError(f"branches is True or False, got {branches!r}")
    if branches and not topology:
        raise ValueError("branches are the segments of the topology's link graph: give topology=True (and measure_threshold) too")
    if polylines is not True and polylines is not False:
        raise ValueError(f"polylines is True or False, got {polylines!r}")
    if polylines and not branches:
        raise ValueError("polylines order the pixels of the branch table's segments: give branches=True (and topology, measure_threshold) too")
    if simplify_px is not None:
        if not polylines:
            raise ValueError("simplify_px simplifies the polylines: give polylines=True (and branches, topology, measure_threshold) too")
        simplify_tolerance(simplify_px, "simplify_px")
    gap = None
    gap_target(bridge_to, "bridge_to")
    if bridge_gap_px is not None:
        if measure_threshold is None or not topology:
            raise ValueError("bridge_gap_px bridges the ends of the topology: give topology=True and measure_threshold too")
        gap = gap_radius(bridge_gap_px, "bridge_gap_px")
    elif bridge_to != "any":
        raise ValueError(f"bridge_to={bridge_to!r} says where bridge_gap_px may bridge to: give bridge_gap_px too")
    measure = None if measure_threshold is None else unit_threshold(measure_threshold, "measure_threshold")
    min_px = None
    if min_crack_px is not None:
        if measure is None:
            raise ValueError("min_crack_px filters what measure_threshold measures: give measure_threshold too")
        min_px = component_min_px(min_crack_px, "min_crack_px")
    radius = None
    if width_radius is not None:
        if measure is None:
            raise ValueError("width_radius measures the skeleton of measure_threshold: give measure_threshold too")
        radius = _width_radius(width_radius, "width_radius")
    spur = None
    if prune_spur_px is not None:
        if measure is None:
            raise ValueError("prune_spur_px prunes the skeleton of measure_threshold: give measure_threshold too")
        spur = spur_length(prune_spur_px, "prune_spur_px")
    saver = None
    if save_dir is not None:
        saver = _Saver(save_dir, thresholds) if measure is None else _Saver(save_dir, thresholds, skeletons=True, bridged=gap is not None)
    stats, instances, widths, topologies, spurs, branch_rows, gap_rows = [], [], [], [], [], [], []
    th32 = torch.tensor([float(t) for t in thresholds], dtype=torch.float32)
    save_th = th32[[i for i in SAVE_THRESHOLD_IDX if i < len(thresholds)]].to(loader.device) if saver is not None else None
    s, dev = loader.scale, loader.device
    want = (s * loader.wh, s * loader.ww)
    for unit in loader:
        sr_u8 = torch.empty(3 * unit.npix, dtype=torch.uint8, device=dev)
        map_u8 = torch.empty(unit.npix, dtype=torch.uint8, device=dev)
        map_f32 = torch.empty(unit.npix, dtype=torch.float32, device=dev)
        kernels = []
        for imgs, a, b in loader.batches(unit):
            dummy = torch.zeros((b - a, 1, ksize, ksize))
            sr_p, seg_p, kernel_preds = model(imgs, dummy)
            if tuple(sr_p.shape) != (b - a, 3, *want) or tuple(seg_p.shape) != (b - a, 1, *want):
                raise ValueError(f"the model returned {tuple(sr_p.shape)} and {tuple(seg_p.shape)} for {b - a} windows of "
                                 f"{loader.wh} x {loader.ww} at scale {s}: expected [n, 3 and 1, {want[0]}, {want[1]}]")
            tiles = loader.stitch_dev[a:b]
            stitch_tiles_u8(sr_p, tiles, loader.off3_dev, loader.out_dims_dev, clip=True, out_u8=sr_u8)
            stitch_tiles_u8(seg_p, tiles, loader.off1_dev, loader.out_dims_dev, clip=False, out_f32=map_f32, out_u8=map_u8)
            kernels.append(kernel_preds.clamp(0, 1).to(torch.float32))
        kernels = torch.cat(kernels)
        layout = [(int(loader.pix_offsets[i]), int(loader.out_dims[i, 0]), int(loader.out_dims[i, 1]),
                   int(loader.tile_start[i]) - unit.t0, int(loader.tile_start[i + 1] - loader.tile_start[i])) for i in range(unit.i0, unit.i1)]
        extra, px, kept_labels, tables, wd2, whist, tmaps, bmaps, btables = [], None, [], None, [], [], [], [], []
        rmaps, ptables, ktables = [], [], []
        gtables, gmaps, glabels = [], [], []
        if measure is not None:
            skel_u8 = torch.empty(unit.npix, dtype=torch.uint8, device=dev)
            bridged_u8 = torch.empty(unit.npix, dtype=torch.uint8, device=dev) if gap is not None else None
            t32 = torch.tensor(measure, dtype=torch.float32, device=dev)
            px, tables = [], []
            for j, (o, H, W, _, _) in enumerate(layout):     # one plane per image: the stitched map, never a tile
                plane = map_f32[o:o + H * W].view(1, H, W)
                sk = skeletonize(plane, measure).view(-1)
                if spur is not None:
                    sk_all = sk
                    sk, spur_n = prune_spurs(sk.view(1, H, W), spur)
                    sk = sk.view(-1)
                if min_px is None:
                    skel_u8[o:o + H * W] = sk * 255
                    px.append(torch.stack([(map_f32[o:o + H * W] - t32 > 0).sum(), sk.sum()]))
                    if spur is not None:
                        px[-1] = torch.cat([px[-1], spur_n.to(torch.int64)])
                    if topology:
                        topo, tints, jl = _topology_ints(sk.view(1, H, W))
                        tmaps.append(topo.view(H, W))
                        px[-1] = torch.cat([px[-1], tints])
                    if gap is not None:                      # the cracks are the components of R
                        lab = label_components(plane, measure)
                        _bridge_into(j, topo, lab, sk, gap, bridge_to, px, gtables, gmaps, glabels, bridged_u8[o:o + H * W], True)
                    d2 = None
                    if radius is not None:
                        d2, hist = skeleton_width(plane, sk.view(1, H, W), measure, radius)
                        wd2.append(d2.view(H, W))
                        whist.append(_hist_and_widest(d2, hist))
                    if branches:
                        bl = label_branches(topo)
                        bmaps.append(bl.view(H, W))
                        btables.append(branch_table(bl, topo, jl, None, d2))
                        btables[-1][:, 0] = j
                        if polylines:
                            _order_into(bl, topo, d2, rmaps, btables, ptables, simplify_px, ktables)
                    continue
                labels = label_components(plane, measure)
                acc = _component_sums(labels, sk)
                keep, kept = _keep_from_sums(labels, acc, min_px, want_labels=True)
                sk = sk * keep.view(-1)                      # skeleton(R) & K = skeleton(K), and prune(skeleton(R)) & K = prune(skeleton(K))
                skel_u8[o:o + H * W] = sk * 255
                table = _table_from_sums(labels, acc, min_px)
                d2 = None
                if spur is not None:                         # per crack: its skeleton pixels before the pruning minus after
                    before = _component_sums(labels, sk_all)[:, 1]
                    table = torch.cat([table, (before - acc[:, 1])[table[:, 0].long(), table[:, 1].long() - 1].view(-1, 1)], 1)
                if radius is not None:                       # against R: for a kept pixel the distance against K is the same
                    d2, hist = skeleton_width(plane, sk.view(1, H, W), measure, radius)
                    wd2.append(d2.view(H, W))
                    whist.append(_hist_and_widest(d2, hist))
                    table = torch.cat([table, _width_columns(table, _component_width(labels, d2), W)], 1)
                px.append(torch.stack([keep.sum(), sk.sum(), (labels != 0).sum()]))
                if spur is not None:
                    px[-1] = torch.cat([px[-1], ((sk_all * keep.view(-1)).sum() - sk.sum()).view(1)])
                if topology:                                 # of the kept skeleton; a removed component has no pixel in it
                    topo, tints, jl = _topology_ints(sk.view(1, H, W))
                    tmaps.append(topo.view(H, W))
                    px[-1] = torch.cat([px[-1], tints])
                    table = torch.cat([table, _topology_columns(table, _component_topology(labels, topo, jl))], 1)
                if gap is not None:                          # the cracks are the kept components
                    _bridge_into(j, topo, kept, sk, gap, bridge_to, px, gtables, gmaps, glabels, bridged_u8[o:o + H * W], False)
                if branches:                                 # a tensor of their own: the topology columns stay the table's last
                    bl = label_branches(topo)
                    bmaps.append(bl.view(H, W))
                    btables.append(branch_table(bl, topo, jl, kept, d2))
                    btables[-1][:, 0] = j
                    if polylines:
                        _order_into(bl, topo, d2, rmaps, btables, ptables, simplify_px, ktables)
                table[:, 0] = j                              # the image within the unit
                tables.append(table)
                kept_labels.append(kept.view(H, W))
            px = torch.stack(px).cpu().tolist()              # the unit's integers in one read
            tables = torch.cat(tables).cpu().numpy() if min_px is not None else None         # and the unit's tables in one more
            whist = torch.stack(whist).cpu().numpy() if radius is not None else None         # the unit's histograms (and widest keys) in one
            btables = torch.cat(btables).cpu().numpy() if branches else None                 # the unit's branch rows in one more
            ptables = torch.cat(ptables).cpu().numpy() if polylines else None                # and the unit's ordered points in one more
            ktables = torch.cat(ktables).cpu().numpy() if simplify_px is not None else None  # and their kept flags in one more
            gtables = torch.cat(gtables).cpu().numpy() if gap is not None else None          # the unit's gap rows in one more
            p_at = 0
            extra = [skel_u8] + ([bridged_u8] if gap is not None else [])
        if saver is not None:
            planes = threshold_planes_u8(map_f32.view(1, -1), save_th)
            saver.push(loader.names[unit.i0:unit.i1], [sr_u8, map_u8, planes, kernels] + extra, layout=layout)
            saver.drain(keep=1)                              # encode the unit before this one while the device runs this one
        for j, (i, (o, H, W, k0, nk)) in enumerate(zip(range(unit.i0, unit.i1), layout)):
            item = {"name": loader.names[i], "sr_u8": sr_u8[3 * o:3 * (o + H * W)].view(H, W, 3), "map_u8": map_u8[o:o + H * W].view(H, W),
                    "map_f32": map_f32[o:o + H * W].view(H, W), "kernels": kernels[k0:k0 + nk]}
            if px is not None:
                crack, skel = int(px[j][0]), int(px[j][1])
                item.update(crack_px=crack, skeleton_px=skel, mean_width_px=mean_width(crack, skel))
                stats.append((loader.names[i], crack, skel, item["mean_width_px"]))
                if min_px is not None:
                    rows = tables[tables[:, 0] == j]
                    cracks = crack_instances(rows[:, :8].tolist(), W)
                    if spur is not None:
                        for c, n in zip(cracks, rows[:, 8].tolist()):
                            c["spur_px"] = n
                    if radius is not None:
                        w0 = 8 if spur is None else 9            # the spur column, where there is one, stands before the width's three
                        for c, (m, y, x) in zip(cracks, rows[:, w0:w0 + 3].tolist()):
                            c.update(max_width_px=width_from_d2(m), widest=(y, x) if m > 0 else None)
                    if topology:
                        for c, sums in zip(cracks, rows[:, -TOPO_ACC:].tolist()):
                            c.update(crack_topology(sums, c["length_px"]))
                    item.update(removed_px=int(px[j][2]) - crack, n_cracks=len(cracks), labels=kept_labels[j], cracks=cracks)
                    instances.append((loader.names[i], cracks))
                if spur is not None:
                    item["spur_px"] = int(px[j][2 if min_px is None else 3])
                    spurs.append((loader.names[i], skel, item["spur_px"]))
                if radius is not None:
                    hist, key = whist[j, :-1], int(whist[j, -1])
                    w = summarize_width_hist(hist, radius)
                    w["widest"] = divmod(H * W - 1 - key % (H * W), W) if key >= H * W else None        # key = max d2 * H W + (H W - 1 - index)
                    item.update({k: w[k] for k in ("max_width_px", "median_width_px", "p95_width_px", "centerline_width_px", "saturated_px",
                                                   "widest")}, width_hist=hist.copy(), width_d2=wd2[j])
                    widths.append((loader.names[i], w))
                if topology:
                    tp = summarize_topology(px[j][-TOPO_COUNTS - 2:-2], px[j][-2], px[j][-1])
                    tp = {k: tp[k] for k in ("endpoints", "junctions", "junction_px", "isolated_px", "loops", "links", "length_geodesic_px",
                                             "orientation")}
                    tp["mean_width_geodesic_px"] = mean_width_geodesic(crack, tp["length_geodesic_px"])
                    item.update(tp, topology_map=tmaps[j])
                    topologies.append((loader.names[i], tp))
                if gap is not None:
                    rows = gtables[gtables[:, 0] == j]
                    bridge_px, n_with_skeleton = (int(v) for v in px[j][-TOPO_COUNTS - 4:-TOPO_COUNTS - 2])     # in front of the topology's twelve
                    of_label = {c["y"] * W + c["x"] + 1: k for k, c in enumerate(item["cracks"])} if min_px is not None else None
                    gs = summarize_gaps(rows, item["n_cracks"] if min_px is not None else n_with_skeleton)
                    glist = crack_gaps(rows, W, of_label)
                    item.update(n_gaps=gs["n_gaps"], n_mutual_gaps=gs["n_mutual"], gap_length_px=gs["gap_length_px"], max_gap_px=gs["max_gap_px"],
                                bridge_px=bridge_px, n_cracks_bridged=gs["n_cracks_bridged"], gaps=glist, bridge_map=gmaps[j], bridged_labels=glabels[j])
                    if min_px is not None:
                        group = gap_group_of(rows)
                        starts = np.bincount([g["crack"] for g in glist], minlength=len(item["cracks"])).tolist()
                        for c, n in zip(item["cracks"], starts):
                            lab = c["y"] * W + c["x"] + 1
                            c.update(group=of_label[group.get(lab, lab)], gaps=n)
                    gap_rows.append((loader.names[i], glist))
                if branches:
                    rows = btables[btables[:, 0] == j]
                    if polylines:                            # the chain flag stands behind the table's columns
                        rows, chain = rows[:, :-1], rows[:, -1]
                    of_label = {c["y"] * W + c["x"] + 1: k for k, c in enumerate(item["cracks"])} if min_px is not None else None
                    blist = crack_branches(rows, W, of_label)
                    kinds = [b["kind"] for b in blist]
                    item.update(n_branches=len(blist), branch_kinds={k: kinds.count(k) for k in BRANCH_KINDS},
                                longest_branch_px=max([b["length_geodesic_px"] for b in blist if b["kind"] != "isolated"], default=0.0),
                                branch_map=bmaps[j], branches=blist)
                    if min_px is not None:
                        per_crack = np.bincount([b["crack"] for b in blist], minlength=len(item["cracks"])).tolist()
                        for c, n in zip(item["cracks"], per_crack):
                            c["n_branches"] = n
                    if polylines:
                        npts = int(rows[chain != 0, 3].sum())                        # px of the chains: the image's span of the unit's points
                        crack_polylines(blist, chain, ptables[p_at:p_at + npts], widths=radius is not None)
                        if simplify_px is not None:
                            nv, total = crack_vertices(blist, ptables[p_at:p_at + npts], ktables[p_at:p_at + npts], widths=radius is not None)
                            item.update(n_vertices=nv, length_simplified_px=total)
                        p_at += npts
                        item.update(n_chains=int((chain != 0).sum()), unordered_branch_px=int(rows[chain == 0, 3].sum()), rank_map=rmaps[j])
                    branch_rows.append((loader.names[i], blist))
            yield item
    if saver is not None:
        saver.drain()
        if measure is not None:
            write_crack_stats(os.path.join(save_dir, "crack_stats.csv"), stats)
        if min_px is not None:
            write_crack_instances(os.path.join(save_dir, "crack_instances.csv"), instances)
        if radius is not None:
            write_crack_widths(os.path.join(save_dir, "crack_widths.csv"), widths)
            if min_px is not None:
                write_crack_instance_widths(os.path.join(save_dir, "crack_instance_widths.csv"), instances)
        if topology:
            write_crack_topology(os.path.join(save_dir, "crack_topology.csv"), topologies)
            if min_px is not None:
                write_crack_instance_topology(os.path.join(save_dir, "crack_instance_topology.csv"), instances)
        if branches:
            write_crack_branches(os.path.join(save_dir, "crack_branches.csv"), branch_rows)
        if polylines:
            write_crack_polylines(os.path.join(save_dir, "crack_polylines.csv"), branch_rows)
        if simplify_px is not None:
            write_crack_vertices(os.path.join(save_dir, "crack_vertices.csv"), branch_rows)
            write_crack_geojson(os.path.join(save_dir, "crack_polylines.geojson"), branch_rows)
        if gap is not None:
            write_crack_gaps(os.path.join(save_dir, "crack_gaps.csv"), gap_rows)
        if spur is not None:
            write_crack_spurs(os.path.join(save_dir, "crack_spurs.csv"), spurs)
            if min_px is not None:
                write_crack_instance_spurs(os.path.join(save_dir, "crack_instance_spurs.csv"), instances)
