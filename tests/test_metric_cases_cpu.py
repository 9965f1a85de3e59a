"""The references and input builders of tests/metric_cases.py, checked before any kernel is involved (no GPU needed):

  * the fp64 restatements reproduce what the reference's own classes produced (tests/golden/aux_reference.npz): the IoU sweep exactly,
    PSNR within 1e-4 dB, SSIM within 1e-5, the blur kernels within 1e-6 of their maximum (the fixture's parameters were rounded to
    fp32 after use, so that one is not bit-equal) -- the tolerances tests/test_aux_rows_gpu.py already uses;
  * every lattice builder's bound holds, so its expected sums are exact in fp32 in any summation order;
  * the IoU tie inputs put, for every threshold, a pixel at t, at nextafter(t, +inf) and at nextafter(t, -inf) into the foreground
    and into the background of every sample of every multi-chunk shape;
  * every C entry point of csrc/data_ops.hip, and each chunked loss reduction, has a row in CASES or a written NOT_COVERED reason.
"""
import os

import numpy as np
import pytest
import torch

import metric_cases as M
from golden_utils import load_golden, max_rel_to_scale

THRESHOLDS = [i * 0.01 for i in range(1, 100)]          # the evaluation loop's sweep


def test_thresholds_are_the_inference_sweep():
    from csbsr_amd.inference import THRESHOLDS as T
    assert T == THRESHOLDS


def test_iou_restatement_reproduces_the_fixture():
    g = load_golden("aux_reference")
    inter, union = M.ref_iou_counts(g["iou_pred"].reshape(2, -1), g["iou_mask"].reshape(2, -1), M.thresholds32(THRESHOLDS))
    assert np.array_equal(M.ref_iou(inter, union), g["iou_sweep"])
    assert inter.dtype == np.int64 and (inter <= union).all() and (np.diff(inter, axis=1) <= 0).all() and (np.diff(union, axis=1) <= 0).all()


def test_psnr_ssim_restatement_reproduces_the_fixture():
    g = load_golden("aux_reference")
    psnr, ssim = M.ref_psnr_ssim(g["met_a"], g["met_b"])
    print("fixture deviation: PSNR %.3g dB, SSIM %.3g" % (np.abs(psnr - g["met_psnr"]).max(), np.abs(ssim - g["met_ssim"]).max()))
    assert np.abs(psnr - g["met_psnr"]).max() < 1e-4
    assert np.abs(ssim - g["met_ssim"]).max() < 1e-5


def test_gaussian_restatement_reproduces_the_fixture():
    g = load_golden("aux_reference")
    k = M.ref_gaussian_kernels(g["deg_params"], 21)
    print("fixture deviation: blur kernels %.3g absolute" % np.abs(k - g["deg_kernels"]).max())
    assert max_rel_to_scale(k, g["deg_kernels"]) < 1e-6
    assert np.abs(k.sum((1, 2)) - 1).max() < 1e-12


@pytest.mark.parametrize("K", M.GAUSS_K)
def test_gaussian_restatement_at_the_corners(K):
    """finite, normalised and symmetric under the point reflection (x, y) -> (-x, -y) at every K and parameter corner of the GPU rows"""
    k = M.ref_gaussian_kernels(M.GAUSS_CORNERS, K)
    assert k.shape == (5, K, K) and np.isfinite(k).all() and (k >= 0).all()
    assert np.abs(k.sum((1, 2)) - 1).max() < 1e-12
    assert np.abs(k - k[:, ::-1, ::-1]).max() < 1e-15


def test_smooth_rounds_within_the_iou_ulp_budget():
    """the kernel adds the fp32 rounding of ``smooth`` where the reference adds the double 1e-5: that moves the quotient by at most
    |fp32(1e-5) / 1e-5 - 1| relative; with the single fp32 rounding of the result (half an ulp, at most 2^-24 relative) the total
    stays within one ulp when the first is below 2^-25"""
    assert abs(float(np.float32(1e-5)) / 1e-5 - 1) < 2.0 ** -25


@pytest.mark.parametrize("N,C,H,W", M.IMG_SHAPES)
def test_psnr_lattice_is_exact(N, C, H, W):
    eq = N - 1 if N > 1 else None
    a, b, sum_sq = M.psnr_lattice(N, C, H, W, seed=H * W, equal_sample=eq)
    assert a.dtype == np.float32 and a.min() >= 0 and a.max() <= 1 and b.min() >= 0 and b.max() <= 1
    d = (a.astype(np.float64) - b.astype(np.float64)) * 256
    assert np.array_equal(d, np.round(d)) and np.abs(d).max() <= 7                      # on the lattice
    assert np.array_equal((a - b).astype(np.float64) * 256, d)                             # the fp32 subtraction is exact
    assert np.array_equal((d * d).reshape(N, -1).sum(1), sum_sq) and sum_sq.max() < M.FP32_EXACT
    want = (sum_sq / 65536.0).astype(np.float32)
    assert np.array_equal(want.astype(np.float64) * 65536, sum_sq)                         # the expected sum is an fp32 number
    if eq is not None:
        assert sum_sq[eq] == 0 and np.isposinf(M.psnr_from_sum_sq(sum_sq, C * H * W)[eq])
    # fp32 sums in two different orders agree with it bit for bit
    sq = ((a - b) * (a - b)).reshape(N, -1)
    assert np.array_equal(np.cumsum(sq, 1, dtype=np.float32)[:, -1], want)
    assert np.array_equal(np.cumsum(sq[:, ::-1], 1, dtype=np.float32)[:, -1], want)
    psnr, _ = M.ref_psnr_ssim(a, b)
    live = sum_sq > 0
    assert np.isposinf(psnr[~live]).all()
    if live.any():
        assert np.abs(psnr[live] - M.psnr_from_sum_sq(sum_sq, C * H * W)[live]).max() < 1e-9


def test_the_large_image_reaches_the_two_level_fold():
    """against the fold's rows-per-chunk as the source has it now: if that grows, this fails instead of the row going single-level"""
    rpc = M.fold_rows_per_chunk()
    rows = [M.partial_rows(C, H, W) for _, C, H, W in M.IMG_SHAPES]
    assert rows[-1] == 1044 and rows[-1] > rpc and max(rows[:-1]) <= rpc and rows[:2] == [1, 3]


@pytest.mark.parametrize("family", ["noise", "smooth"])
@pytest.mark.parametrize("N,C,H,W", M.IMG_SHAPES)
def test_fp32_ssim_stays_near_fp64_on_these_inputs(family, N, C, H, W):
    """the GPU rows' tolerance (1e-5) is about the kernel only if a plain fp32 evaluation of the same formulas sits well inside it on
    the same inputs: a tenth of it is asked here (measured: at most 1.6e-7; 2.3e-7 over other seeds)"""
    a, b = M.ssim_pair(family, N, C, H, W, seed=H + W)
    assert a.dtype == np.float32 and a.min() >= 0 and a.max() <= 1 and b.min() >= 0 and b.max() <= 1
    dev = np.abs(M.ref_psnr_ssim(a, b)[1] - M.ref_psnr_ssim(a, b, dtype=torch.float32)[1]).max()
    print(f"{family} {N}x{C}x{H}x{W}: fp32 vs fp64 SSIM {dev:.3g}")
    assert dev < 1e-6


def test_one_wrong_pixel_moves_the_small_ssim_rows():
    """at the shapes below the fold's threshold a single pixel off by 0.1 moves the mean SSIM by more than the tolerance"""
    for N, C, H, W in M.IMG_SHAPES[:5]:
        a, b = M.ssim_pair("smooth", N, C, H, W, seed=H + W)
        ref = M.ref_psnr_ssim(a, b)[1]
        a2 = a.copy()
        a2[0, 0, 0, W - 1] += np.float32(0.1) if a2[0, 0, 0, W - 1] < 0.5 else np.float32(-0.1)
        assert abs(M.ref_psnr_ssim(a2, b)[1][0] - ref[0]) > 1e-5, (N, C, H, W)


@pytest.mark.parametrize("B,hw,T", [(B, hw, 99) for B, hw in M.IOU_SHAPES] + M.IOU_EXTRA_T)
def test_iou_tie_inputs(B, hw, T):
    th = M.thresholds32(THRESHOLDS) if T == 99 else M.many_thresholds(T)
    assert len(th) == T and np.all(th[1:] > th[:-1])
    pred, mask = M.iou_tie_inputs(B, hw, th, seed=hw + T)
    assert pred.shape == mask.shape == (B, hw) and pred.dtype == mask.dtype == np.float32
    assert set(np.unique(mask).tolist()) <= set(M.MASK_VALUES.tolist())
    if hw >= 65536:          # every chunked shape: each sample holds every tie on both sides of the mask, and every special value
        for n in range(B):
            assert M.tie_coverage_gaps(pred[n], mask[n], th) == [], (n, M.tie_coverage_gaps(pred[n], mask[n], th)[:4])
            assert np.isnan(pred[n]).any() and np.isposinf(pred[n]).any() and np.isneginf(pred[n]).any()
            for v in (0.0, 1.0, -0.25, 1.5):
                assert (pred[n] == np.float32(v)).any()
            assert set(np.unique(mask[n]).tolist()) == set(M.MASK_VALUES.tolist())
    inter, union = M.ref_iou_counts(pred, mask, th)
    fg = (mask > np.float32(0.5)).sum(1)
    assert (inter <= fg[:, None]).all() and (union >= fg[:, None]).all() and (union <= hw).all()
    # a tie decided the other way changes the union: `>=` in place of `>` is visible in every sample of every shape (the single pixel
    # of (1, 1) is a background pixel AT the lowest threshold), and at every threshold of the chunked shapes
    with np.errstate(invalid="ignore"):
        u_ge = np.stack([(((pred - t) >= 0) | (mask > np.float32(0.5))).sum(1) for t in th], 1)
    assert (u_ge >= union).all() and (u_ge != union).any(1).all()
    if hw >= 65536:
        assert (u_ge > union).all()


def test_iou_background_sample():
    th = M.thresholds32(THRESHOLDS)
    pred, mask = M.iou_tie_inputs(2, 65537, th, seed=5, background_sample=1)
    inter, union = M.ref_iou_counts(pred, mask, th)
    assert (inter[1] == 0).all() and (union[1] == 0).all() and (M.ref_iou(inter, union)[1] == 1.0).all()
    assert (pred[1] == th[0]).any() and (union[0] > 0).all()


def test_l1_lattice_is_exact():
    c = M.l1_lattice()
    N, C, hw = M.L1_SHAPE
    assert C * hw == 66789 and (C * hw + 65535) // 65536 == 2
    per = (C * hw + 1) // 2
    assert hw < per < 2 * hw                                     # the chunk boundary falls inside plane 1
    d = c["a"].astype(np.float64) - c["b"].astype(np.float64)
    w = c["wmap"].astype(np.float64)[:, None, :]
    assert np.array_equal(d * 256, np.round(d * 256)) and np.abs(d * 256).max() <= 15 and set(np.unique(w * 4).tolist()) == {2, 3, 4, 5, 6}
    tw, t1 = (w * np.abs(d)).reshape(N, -1).sum(1), np.abs(d).reshape(N, -1).sum(1)          # exact in fp64: < 2^24 units of 2^-10
    assert tw.max() * 1024 < M.FP32_EXACT and tw.max() <= 5870.5
    assert np.array_equal(c["sums_w"].astype(np.float64), tw) and np.array_equal(c["sums_1"].astype(np.float64), t1)
    for key, wt in (("da_w", w), ("da_1", np.ones_like(w))):
        want = c["gscale"] * c["gs_n"].astype(np.float64)[:, None, None] * wt * np.sign(d)
        assert np.array_equal(c[key].astype(np.float64), want)
        acc = c["da0"].astype(np.float64) + want
        assert np.array_equal((c["da0"] + c[key]).astype(np.float64), acc)                   # the accumulate path adds exactly
    assert (c["da_w"] == 0).sum() > 1000 and (c["da_w"] > 0).any() and (c["da_w"] < 0).any()
    # a wmap indexed without the wrap at the plane boundary (i in place of i % hw) or a dropped tail would change the sums
    assert not np.array_equal(np.roll(c["wmap"], 1, axis=1), c["wmap"])


def test_plane_lattice_is_exact():
    c = M.plane_lattice()
    planes, hw = M.PLANE_SHAPE
    assert (hw + 65535) // 65536 == 2 and (hw + 1) // 2 == 33033
    a, b = c["a"].astype(np.float64), c["b"].astype(np.float64)
    assert np.array_equal(a * 256, np.round(a * 256)) and a.min() >= 0 and a.max() * 256 <= 12 and b.max() * 256 <= 12
    assert (a * a).sum(1).max() * 65536 < M.FP32_EXACT
    assert np.array_equal(c["sum_a"].astype(np.float64), a.sum(1)) and np.array_equal(c["sum_aa"].astype(np.float64), (a * a).sum(1))
    assert np.array_equal(c["sum_ab"].astype(np.float64), (a * b).sum(1))
    assert np.array_equal(np.cumsum(c["a"] * c["b"], 1, dtype=np.float32)[:, -1], c["sum_ab"])


def test_segloss_inputs():
    p, t = M.segloss_inputs()
    N, H, W = M.SEG_SHAPE
    assert H * W == 66065 and tuple(p.shape) == (N, 1, H, W)
    assert int((p == 0).sum()) >= 14 and float(t[1].sum()) == 0 and float(t[0].sum()) > 1000
    flat = p[1].reshape(-1)
    assert float(flat[33032]) == 0 and float(flat[33033]) == 0      # zeros on both sides of the chunk boundary


# ------------------------------------------------------------------------------------------- coverage

def test_every_entry_point_has_a_row_or_a_reason():
    names = M.data_ops_entry_points()
    assert names == ["csbsr_gaussian_kernels", "csbsr_iou_sweep", "csbsr_psnr_ssim"]
    for name, src in M.LOSS_ENTRY_POINTS.items():
        with open(os.path.join(M.CSRC, src)) as f:
            assert f'extern "C" int {name}(' in f.read(), f"{name} is not an entry point of {src}"
    miss = M.missing_entry_points(M.CASES, M.NOT_COVERED)
    assert not miss, "entry points without a row in tests/metric_cases.py (add one, or a NOT_COVERED reason): " + ", ".join(miss)
    for name, why in M.NOT_COVERED.items():
        assert isinstance(why, str) and len(why.split()) >= 6, f"NOT_COVERED[{name}] needs a written reason"
        assert not M.CASES.get(name), f"NOT_COVERED[{name}] has rows"


def test_case_rows_exist_in_the_gpu_module():
    with open(os.path.join(M.ROOT, "tests", "test_metrics_exact_gpu.py")) as f:
        src = f.read()
    for name, rows in M.CASES.items():
        for r in rows:
            assert f"\ndef {r}(" in src, f"CASES[{name}] names {r}, which tests/test_metrics_exact_gpu.py does not define"
        assert f'"{name}"' in src, f"tests/test_metrics_exact_gpu.py never calls {name}"


def test_the_check_names_a_missing_entry_point():
    """a new entry point in data_ops.hip, a dropped row list or a dropped loss reduction fails the check by name"""
    with open(os.path.join(M.CSRC, "data_ops.hip")) as f:
        text = f.read() + '\nextern "C" int csbsr_next_metric(const float* a, csbsr_stream_t s) { return 0; }\n'
    grown = M.data_ops_entry_points(text) + list(M.LOSS_ENTRY_POINTS)
    assert M.missing_entry_points(M.CASES, M.NOT_COVERED, grown) == ["csbsr_next_metric"]
    assert M.missing_entry_points(M.CASES, {"csbsr_next_metric": "a reason of at least six words"}, grown) == []
    cases = {k: v for k, v in M.CASES.items() if k != "csbsr_plane_reduce"}
    assert M.missing_entry_points(cases, M.NOT_COVERED) == ["csbsr_plane_reduce"]
    cases = dict(M.CASES, csbsr_iou_sweep=[])
    assert M.missing_entry_points(cases, M.NOT_COVERED) == ["csbsr_iou_sweep"]
