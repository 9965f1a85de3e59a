"""Tolerant precision / recall / F without a GPU: the two NumPy restatements of csbsr_pr_sweep against each other on every case of the
GPU tests, the C ABI, pr_scores / summarize_pr against naive loops and a hand-made example, and the evaluation drivers' defaults."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import pr_sweep_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(PC.cases()))
def test_the_two_restatements_agree(name):
    pred, mask, th, tol2 = PC.cases()[name]
    a, b = PC.counts_per_threshold(pred, mask, th, tol2), PC.counts_histogram(pred, mask, th, tol2)
    assert a.dtype == b.dtype == np.int64 and a.shape == (pred.shape[0], 4, len(th))
    assert np.array_equal(a, b), np.argwhere(a != b)[:5]
    assert (np.diff(a[:, :3], axis=2) <= 0).all() and (a[:, 1] <= a[:, 0]).all() and (a[:, 2] <= a[:, 3]).all()      # nested masks


def test_the_two_restatements_agree_at_the_realistic_size():
    pred, mask, th, tol2 = PC.realistic()
    want = PC.realistic_reference()
    assert np.array_equal(want, PC.counts_histogram(pred, mask, th, tol2))
    gt = mask > 0.5
    assert 0.002 < gt.mean() < 0.1 and len(np.unique(want[:, 0])) > 150                # sparse cracks, a map with many distinct levels
    assert (want[:, 1] < want[:, 0]).any() and (want[:, 2] < want[:, 3]).any() and (want[:, 2] > 0).any()
    strict = PC.counts_histogram(pred, mask, th, 0)
    assert (strict[:, 1] < want[:, 1]).any() and (strict[:, 2] < want[:, 2]).any()     # the tolerance matters on these maps


def test_the_cases_hold_what_they_are_meant_to():
    c = PC.cases()
    t32 = PC.th32(PC.THRESHOLDS)
    for name in ("37x70_tol2_4", "33x129_tol2_25"):
        pred, mask, _, _ = c[name]
        H, W = pred.shape[1:]
        gt = mask[0] > 0.5
        assert gt[0].any() and gt[-1].any() and gt[:, 0].any() and gt[:, -1].any()     # all four borders
        assert gt[:, PC.SEAM_X - 1].any() and gt[:, PC.SEAM_X].any() and gt[PC.SEAM_Y - 1].any() and gt[PC.SEAM_Y].any()
        lv = PC.levels(pred[0], t32)
        assert lv[0].any() and lv[-1].any() and lv[:, 0].any() and lv[:, -1].any()
        assert lv[PC.SEAM_Y - 1:PC.SEAM_Y + 1, PC.SEAM_X - 1:PC.SEAM_X + 1].all()
        assert np.isnan(pred).any() and np.isin(t32, pred).all()                        # NaN; every threshold met exactly
        assert (mask == np.float32(0.5)).any() and (mask == np.float32(0.51)).any()
        assert not gt[mask[0] == np.float32(0.5)].any() and gt[mask[0] == np.float32(0.51)].all()
    for tol2 in PC.TOL2:
        pred, mask, th, t2 = c[f"boundary_tol2_{tol2}"]
        by_column = lambda a: a[np.argsort(a[:, 1])]
        (g0, g1), (p0, p1) = by_column(np.argwhere(mask[0] > 0.5)), by_column(np.argwhere(pred[0] > 0.5))
        d = [int(((g - p) ** 2).sum()) for g, p in ((g0, p0), (g1, p1))]
        assert t2 == tol2 and d[0] == tol2 and d[1] > tol2
        assert all(not (a * a + b * b == k) for k in range(tol2 + 1, d[1]) for a in range(18) for b in range(18))    # the next sum of squares
        assert g0[1] == PC.SEAM_X - 1 and (p0[1] >= PC.SEAM_X or tol2 == 0) and g1[1] == 2 * PC.SEAM_X - 1
        assert p1[1] >= 2 * PC.SEAM_X or p1[0] >= PC.SEAM_Y
        assert PC.counts_histogram(pred, mask, th, tol2)[0, :, 0].tolist() == [2, 1, 1, 2]
    assert len(PC.cases()["T255"][2]) == 255 and len(PC.cases()["T1"][2]) == 1 and PC.cases()["batch3"][0].shape == (3, 33, 129)
    b = PC.cases()["batch3"]
    per = PC.counts_histogram(*b)
    assert len({per[i].tobytes() for i in range(3)}) == 3                               # three different images


def test_abi_matches_the_header():
    from csbsr_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    decl = re.search(r"int\s+csbsr_pr_sweep\s*\(([^)]*)\)\s*;", hdr)
    assert decl, "csbsr_pr_sweep is not declared in include/csbsr_hip.h"
    ctype = {"const float*": L.vp, "uint32_t*": L.vp, "int32_t*": L.vp, "csbsr_stream_t": L.vp, "int32_t": L.i32}
    args = [ctype[" ".join(a.split()[:-1])] for a in decl.group(1).replace("\n", " ").split(",")]
    res, sig = L.SIGNATURES["csbsr_pr_sweep"]
    assert res is L.i32 and sig == args and len(args) == 11
    assert "pr_sweep.hip" in open(os.path.join(ROOT, "csbsr_amd", "csrc", "Makefile")).read()


def test_tolerance_to_squared_radius():
    from csbsr_amd.utils.estimate_metrics import pr_sweep, pr_tol2
    assert [pr_tol2(t) for t in (0, 1, 1.5, 2.0, 2.24, 2.9, 5, 16)] == [0, 1, 2, 4, 5, 8, 25, 256]
    for bad in (-0.5, 16.01, 100, float("nan")):
        with pytest.raises(ValueError):
            pr_tol2(bad)
        with pytest.raises(ValueError):                                                 # refused before the library is touched
            pr_sweep(torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), PC.THRESHOLDS, tolerance=bad)
    assert inspect.signature(pr_sweep).parameters["tolerance"].default == 2.0


def _random_counts(seed, N, T):
    rng = np.random.default_rng(seed)
    n_pred = np.sort(rng.integers(0, 500, size=(N, T)), axis=1)[:, ::-1]
    n_gt = np.repeat(rng.integers(1, 300, size=(N, 1)), T, axis=1)
    tp_pred = (n_pred * rng.random((N, T))).astype(np.int64)
    tp_gt = np.sort((n_gt * rng.random((N, T))).astype(np.int64), axis=1)[:, ::-1]      # recall falls with the threshold
    return np.stack([n_pred, tp_pred, tp_gt, n_gt], axis=1).astype(np.int64)


def test_scores_equal_the_naive_loops():
    from csbsr_amd.inference import pr_scores, summarize_pr
    c = _random_counts(0, 5, 99)
    c[1, :, 90:] = 0                   # nothing predicted and no match at the high thresholds of image 1
    c[2, 3] = 0                        # image 2 has no ground truth
    c[2, 2] = 0
    c[3, 1:3] = 0                      # image 3 matches nothing: P = R = 0
    got, want = pr_scores(c), PC.scores_naive(c)
    for g, w in zip(got, want):
        assert g.dtype == np.float64 and g.shape == (5, 99) and np.array_equal(g, np.array(w))
    p, r, f = got
    assert (p[1, 90:] == 1).all() and (r[2] == 1).all() and (f[3] == 0).all() and (p[3][c[3, 0] > 0] == 0).all()
    s, w = summarize_pr(c, PC.THRESHOLDS), PC.summary_naive(c, PC.THRESHOLDS)
    assert list(s) == ["ODS", "ODS_threshold", "OIS", "AP", "P_at_ODS", "R_at_ODS"] and all(isinstance(v, float) for v in s.values())
    for k in ("ODS", "ODS_threshold", "P_at_ODS", "R_at_ODS"):
        assert s[k] == w[k], k
    # sums of at most 98 terms in [0, 1] (AP) and of 5 (OIS) in another order: a few ulps of 1
    assert abs(s["AP"] - w["AP"]) <= 98 * 2.0 ** -52 and abs(s["OIS"] - w["OIS"]) <= 5 * 2.0 ** -52
    # the degenerate conventions one by one
    p, r, f = pr_scores(np.array([[[0, 0], [0, 0], [0, 3], [0, 4]]]))
    assert p.tolist() == [[1.0, 1.0]] and r.tolist() == [[1.0, 0.75]] and f.tolist() == [[1.0, 2 * 0.75 / 1.75]]
    p, r, f = pr_scores(np.array([[[5], [0], [0], [7]]]))
    assert (p[0, 0], r[0, 0], f[0, 0]) == (0.0, 0.0, 0.0)


def test_summary_of_a_hand_made_example():
    """Two images, three thresholds.  Rows: n_pred, tp_pred, tp_gt, n_gt.
      image A: P = 4/8, 3/4, 1/1   R = 8/8, 6/8, 2/8   F = 2/3, 3/4, 2/5          best F 3/4
      image B: P = 2/8, 2/4, 0/0=1 R = 2/2, 1/2, 0/2   F = 2/5, 1/2, 0            best F 1/2
      dataset: n_pred 16, 8, 1; tp_pred 6, 5, 1; tp_gt 10, 7, 2; n_gt 10
               P = 3/8, 5/8, 1     R = 1, 7/10, 1/5    F = 6/11, 35/53, 1/3
      ODS = 35/53 at the second threshold; OIS = (3/4 + 1/2) / 2 = 5/8;
      AP  = (1 - 7/10)(3/8 + 5/8)/2 + (7/10 - 1/5)(5/8 + 1)/2 = 3/20 + 13/32 = 89/160."""
    from csbsr_amd.inference import pr_scores, summarize_pr
    a = [[8, 4, 1], [4, 3, 1], [8, 6, 2], [8, 8, 8]]
    b = [[8, 4, 0], [2, 2, 0], [2, 1, 0], [2, 2, 2]]
    c = np.array([a, b])
    p, r, f = pr_scores(c)
    assert np.allclose(f, [[2 / 3, 3 / 4, 2 / 5], [2 / 5, 1 / 2, 0.0]], rtol=0, atol=1e-15) and p[1, 2] == 1.0 and r[1, 2] == 0.0
    s = summarize_pr(c, [0.25, 0.5, 0.75])
    assert s["ODS_threshold"] == 0.5 and s["P_at_ODS"] == 5 / 8 and s["R_at_ODS"] == 7 / 10
    for k, v in (("ODS", 35 / 53), ("OIS", 5 / 8), ("AP", 89 / 160)):
        assert abs(s[k] - v) <= 4 * 2.0 ** -52, k


@pytest.mark.parametrize("name", ["37x70_tol2_0", "33x129_tol2_0", "T255"])
def test_tolerance_zero_is_the_iou_of_the_binarised_maps(name):
    pred, mask, th, _ = PC.cases()[name]
    c = PC.counts_histogram(pred, mask, th, 0)
    assert np.array_equal(c[:, 1], c[:, 2])                                             # one intersection
    t32 = PC.th32(th)
    for j in range(0, len(th), 7):
        with np.errstate(invalid="ignore"):
            p = (pred - t32[j]) > 0
        g = mask > 0.5
        inter, uni = (p & g).sum(axis=(1, 2)), (p | g).sum(axis=(1, 2))
        assert np.array_equal(c[:, 1, j], inter) and np.array_equal(c[:, 0, j] + c[:, 3, j] - c[:, 1, j], uni)
        assert np.array_equal(c[:, 1, j] / (c[:, 0, j] + c[:, 3, j] - c[:, 1, j]), inter / uni)


def test_csv_layout(tmp_path):
    from csbsr_amd.inference import pr_scores, write_pr_log
    c = _random_counts(3, 4, 99)
    c[0, :, 95:] = 0
    names = [f"img_{i}.png" for i in range(4)]
    path = tmp_path / "pr_log.csv"
    write_pr_log(str(path), c, PC.THRESHOLDS, names)
    fn, th, p, r, f = PC.read_pr_log(str(path))
    assert fn == names and th == PC.THRESHOLDS
    for got, want in zip((p, r, f), pr_scores(c)):
        assert np.array_equal(got, want)
    lines = open(path).read().splitlines()
    assert len(lines) == 1 + 3 * 4 and lines[0].startswith(",,0.01,") and lines[1].startswith("img_0.png,P,") and lines[3].startswith("img_0.png,F,")


# ------------------------------------------------------------------------------------------------ the drivers, over CPU stand-ins
def _stand_ins(monkeypatch):
    """evaluate_dataset / evaluate_batch have no CPU path: their device calls are replaced by plain torch stand-ins (the host logic --
    accumulation, keys, summary, files -- is what runs), pr_sweep by the restatement."""
    from csbsr_amd import inference as I

    def stitch(p, shape, clip, want_f32=True, want_u8=False):
        s = [int(v) for v in shape]
        nH, nW, Cc, ph, pw = s[2:]
        B = p.shape[0] // (nH * nW)
        f = p.view(B, nH, nW, Cc, ph, pw).permute(0, 3, 1, 4, 2, 5).reshape(B, Cc, nH * ph, nW * pw)
        f = f.clamp(0, 1) if clip else f
        return f, (f.clamp(0, 1).mul(255).byte().permute(0, 2, 3, 1).contiguous() if want_u8 else None)

    def iou(seg, masks, thresholds, smooth=1e-5):
        t = torch.tensor([float(v) for v in thresholds]).view(1, -1, 1)
        b, g = (seg.reshape(seg.shape[0], 1, -1) - t) > 0, masks.reshape(masks.shape[0], 1, -1) > 0.5
        return (((b & g).sum(2) + smooth) / ((b | g).sum(2) + smooth)).float()

    calls = []

    def pr(seg, masks, thresholds, tolerance=2.0):
        calls.append(tolerance)
        H, W = seg.shape[-2:]
        c = PC.counts_histogram(seg.reshape(-1, H, W).numpy(), masks.reshape(-1, H, W).numpy(), thresholds, int(tolerance * tolerance))
        return torch.from_numpy(c.astype(np.int32))

    monkeypatch.setattr(I, "stitch_clip_u8", stitch)
    monkeypatch.setattr(I, "psnr_ssim", lambda a, b: ((a - b).flatten(1).pow(2).mean(1), (a * b).flatten(1).mean(1)))
    monkeypatch.setattr(I, "iou_sweep", iou)
    monkeypatch.setattr(I, "pr_sweep", pr)
    monkeypatch.setattr(I, "_Saver", lambda d, th: os.makedirs(d))            # no image files: the ring of pinned slots needs the device
    return I, calls


def _cpu_batches():
    import eval_io_cases as EC
    hr, masks, lr, kernels, names = EC.make_testset(11, 4, 64, 96, 4, zero_mask=3)
    items = [EC.reference_item_numpy(hr[i], masks[i], lr[i], kernels[i], (32, 48), 4, 2) for i in range(4)]
    out = []
    for i0 in (0, 2):
        col = lambda k: torch.from_numpy(np.stack([it[k] for it in items[i0:i0 + 2]]))
        out.append((col(0), col(1), col(2), col(3), [n.replace("jpg", "png") for n in names[i0:i0 + 2]], items[i0][4], items[i0][5]))
    return out


TODAY = {"fnames", "psnr", "ssim", "kernel_psnr", "iou", "summary"}
TODAY_SUMMARY = {"PSNR_mean", "SSIM_mean", "PSNR(Kernel)_mean", "AIU_mean", "IoU_max"}
PR_SUMMARY = {"ODS", "ODS_threshold", "OIS", "AP", "P_at_ODS", "R_at_ODS"}


def test_the_drivers_default_to_no_pr_metrics(monkeypatch, tmp_path):
    import eval_io_cases as EC
    I, calls = _stand_ins(monkeypatch)
    for fn in (I.evaluate_dataset, I.evaluate_batch):
        assert inspect.signature(fn).parameters["pr_tolerance"].default is None
    batches = _cpu_batches()
    plain = I.evaluate_dataset(EC.stub_model, batches, save_dir=str(tmp_path / "plain"))
    assert set(plain) == TODAY and set(plain["summary"]) == TODAY_SUMMARY and calls == []
    assert os.listdir(tmp_path / "plain") == ["iou_log.csv"]

    out = I.evaluate_dataset(EC.stub_model, batches, pr_tolerance=2, save_dir=str(tmp_path / "pr"))
    assert set(out) == TODAY | {"pr_counts"} and set(out["summary"]) == TODAY_SUMMARY | PR_SUMMARY and calls == [2, 2]
    assert out["pr_counts"].dtype == np.int64 and out["pr_counts"].shape == (4, 4, 99)
    assert out["iou"].tobytes() == plain["iou"].tobytes() and {k: out["summary"][k] for k in TODAY_SUMMARY} == plain["summary"]
    assert {k: out["summary"][k] for k in PR_SUMMARY} == I.summarize_pr(out["pr_counts"], I.THRESHOLDS)
    assert (out["pr_counts"][3, 3] == 0).all() and (I.pr_scores(out["pr_counts"])[1][3] == 1).all()       # image 3: the empty mask
    assert sorted(os.listdir(tmp_path / "pr")) == ["iou_log.csv", "pr_log.csv"]
    fn, th, p, r, f = PC.read_pr_log(str(tmp_path / "pr" / "pr_log.csv"))
    assert fn == out["fnames"] and all(np.array_equal(a, b) for a, b in zip((p, r, f), I.pr_scores(out["pr_counts"])))

    imgs, sr_t, m, kt, _, s1, s2 = batches[0]
    monkeypatch.setattr(I, "JointPatch", lambda: (lambda p, shape: I.stitch_clip_u8(p, shape, clip=False)[0]))
    b0 = I.evaluate_batch(EC.stub_model, imgs, s1, s2, sr_t, m, kt, ksize=21)
    assert set(b0) == {"sr_preds", "segment_preds", "kernel_preds", "psnr", "ssim", "kernel_psnr", "iou"}
    b1 = I.evaluate_batch(EC.stub_model, imgs, s1, s2, sr_t, m, kt, ksize=21, pr_tolerance=2)
    assert set(b1) == set(b0) | {"pr_counts"} and np.array_equal(b1["pr_counts"], out["pr_counts"][:2]) and b1["pr_counts"].dtype == np.int64

    for bad in (-1, 17):                                                                # refused before the model runs
        with pytest.raises(ValueError):
            I.evaluate_dataset(lambda *a, **k: pytest.fail("the model ran"), batches, pr_tolerance=bad)
