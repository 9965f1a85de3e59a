"""Generate the surface-distance fixture from the REFERENCE's own code: the vendored ``surface_distance`` package
(/root/reference/model/utils/metrics/surface_distance), driven per (image, threshold) cell the way calc_distance_metrics
(model/engine/inference.py:293-336) drives it, run on CPU in the build container.

    python tests/golden/make_surface_golden.py          # rewrites tests/golden/surface_distance.npz

Only data is written: probability maps (uint8, value k / 255 in fp32), masks, the 99 thresholds, the reference's HD / MSD per cell and
its outlier counts, its 16-entry contour-length table, per cell the margin of the percentile decision, and its seconds per image.
"""
import os
import sys
import time

import numpy as np
from scipy import ndimage

if not hasattr(np, "Inf"):
    np.Inf = np.inf          # the package predates numpy 2

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
from model.utils.metrics.surface_distance.metrics import surface_distance as SD, lookup_tables  # noqa: E402

THRESHOLDS = [i * 0.01 for i in range(1, 100)]           # inference.py:50
PERCENT = 50                                             # inference.py:302
TIE = 1e-9


def smooth_field(rng, h, w, sigma):
    f = ndimage.gaussian_filter(rng.standard_normal((h, w)), sigma, mode="wrap")
    return (f - f.min()) / (f.max() - f.min())


def random_case(seed, h, w, gain=1.0):
    """a smooth probability map (gain > 1: saturating at both ends, so the far thresholds keep large regions) and a mask that resembles
    its level set without following it"""
    rng = np.random.default_rng(seed)
    f = smooth_field(rng, h, w, 6.0)
    prob = np.round(255 * np.clip(gain * (f + 0.08 * smooth_field(rng, h, w, 2.0) - 0.54) + 0.5, 0, 1)).astype(np.uint8)
    mask = (f + 0.25 * (smooth_field(rng, h, w, 4.0) - 0.5) > 0.55).astype(np.uint8)
    return prob, mask


def hand_cases(h=48, w=80):
    rng = np.random.default_rng(5)
    blob = np.round(255 * smooth_field(rng, h, w, 5.0)).astype(np.uint8)
    zeros = np.zeros((h, w), np.uint8)
    rect = zeros.copy()
    rect[10:30, 20:50] = 1
    corner = zeros.copy()
    corner[:17, :23] = 1                                  # touches the top and the left image edge
    shifted = np.roll(np.roll(rect, 5, 0), -7, 1)
    return {
        "empty_empty": (zeros, zeros),
        "empty_nonempty": (blob, zeros),                  # (prediction, gt): gt empty, prediction not
        "nonempty_empty": (zeros, rect),
        "all_ones": (np.full((h, w), 255, np.uint8), np.ones((h, w), np.uint8)),
        "two_edges": (blob, corner),
        "two_edges_same": ((200 * corner).astype(np.uint8), corner),
        "shifted": ((200 * shifted).astype(np.uint8), rect),
    }


def margin_of(areas):
    cum = np.cumsum(areas) / np.sum(areas)
    return float(np.min(np.abs(cum - PERCENT / 100.0)))


def run_reference(prob_u8, mask_u8):
    """one image through the 99 thresholds; returns hd [T], msd [T], margin [T], outlier counts, seconds"""
    prob = prob_u8.astype(np.float32) / np.float32(255)
    th = np.asarray(THRESHOLDS, np.float32)                # torch.Tensor(thresholds)
    preds = (prob[None] - th[:, None, None]) > 0           # inference.py:112, fp32
    gt = mask_u8.astype(np.float32) > 0.5
    max_img_len = prob.shape[1]                            # np.max(preds.shape[3:]) of [B, T, H, W]: the width
    T = len(THRESHOLDS)
    hd, msd, margin = np.zeros(T), np.zeros(T), np.full(T, np.inf)
    n_hd = n_msd = 0
    t0 = time.perf_counter()
    cells = []
    for j in range(T):
        s = SD.compute_surface_distances(gt, preds[j], spacing_mm=(1, 1))
        cells.append(s)
        g2p, p2g = s["distances_gt_to_pred"], s["distances_pred_to_gt"]
        ag, ap = s["surfel_areas_gt"], s["surfel_areas_pred"]
        if len(g2p) == 0 and len(p2g) == 0:
            hd[j] = 0
        elif len(g2p) == 0 or len(p2g) == 0:
            hd[j] = max_img_len
            n_hd += 1
        else:
            hd[j] = SD.compute_robust_hausdorff(s, PERCENT)
        if np.sum(ag) == 0 and np.sum(ap) == 0:
            msd[j] = 0
        elif np.sum(ag) == 0 or np.sum(ap) == 0:
            msd[j] = max_img_len
            n_msd += 1
        else:
            a, b = SD.compute_average_surface_distance(s)
            msd[j] = (a + b) / 2
    seconds = time.perf_counter() - t0
    for j, s in enumerate(cells):                          # outside the timed loop
        if len(s["distances_gt_to_pred"]) and len(s["distances_pred_to_gt"]):
            margin[j] = min(margin_of(s["surfel_areas_gt"]), margin_of(s["surfel_areas_pred"]))
    return hd, msd, margin, n_hd, n_msd, seconds


def main():
    out = dict(thresholds=np.asarray(THRESHOLDS, np.float64), percent=np.float64(PERCENT), tie_margin=np.float64(TIE),
               length_table=np.asarray(lookup_tables.create_table_neighbour_code_to_contour_length((1, 1)), np.float64))
    # Smooth closed contours land on exact percentile ties in 3 .. 7 % of their cells (the reference alone decides that: cum_k / total ==
    # 1/2 exactly); these seeds were picked, by running the reference only, to stay under the 5 % the check below allows.
    cases = {"rand_96x160": random_case(16, 96, 160), "rand_128x128": random_case(12, 128, 128, gain=2.0),
             "rand_61x203": random_case(15, 61, 203)}
    random_names = list(cases)
    cases.update(hand_cases())
    ties = cells = 0
    for name, (prob, mask) in cases.items():
        hd, msd, margin, n_hd, n_msd, sec = run_reference(prob, mask)
        out.update({f"prob_{name}": prob, f"mask_{name}": mask, f"hd_{name}": hd, f"msd_{name}": msd, f"margin_{name}": margin,
                    f"hd_outliers_{name}": np.int64(n_hd), f"msd_outliers_{name}": np.int64(n_msd), f"seconds_{name}": np.float64(sec)})
        t = int((margin < TIE).sum())
        print(f"{name:16s} {prob.shape}  ties {t:2d}  outliers {n_hd}/{n_msd}  hd {hd.min():.3f}..{hd.max():.3f}  "
              f"msd {msd.min():.3f}..{msd.max():.3f}  {sec:.2f} s")
        if name in random_names:
            ties += t
            cells += len(margin)
    assert ties <= 0.05 * cells, f"{ties} of {cells} random cells are percentile ties: choose other seeds"
    out.update(cases=np.array(list(cases)), random_cases=np.array(random_names))
    path = os.path.join(HERE, "surface_distance.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote", path, os.path.getsize(path), "bytes;", ties, "ties in", cells, "random cells")


if __name__ == "__main__":
    main()
