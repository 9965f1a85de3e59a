"""Thinning and clDice without a GPU: the NumPy restatement of tests/skeleton_cases.py on the literal patterns, its invariants on every case
of the GPU tests (subset, idempotence, 8-connectivity), the tiling argument the kernel rests on, the score conventions, the CSV writers,
the C ABI and the argument refusals."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import skeleton_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("csbsr_skeleton_max_passes", "csbsr_skeleton_init", "csbsr_skeleton_passes", "csbsr_skeleton_finish", "csbsr_centerline_counts")


def _bin(name):
    return SC.cases()[name] > 0.5


# ------------------------------------------------------------------------------------------------ the rule on literal patterns
def test_lines_and_tiny_planes_come_back_unchanged():
    for name in ("1x1_set", "1x1_clear", "1xW_line", "Hx1_line", "zeros"):
        assert np.array_equal(SC.expected(name), _bin(name)), name
    assert SC.expected("3x3_full")[0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert SC.expected("3x3_cross").sum() == 2


def test_literal_patterns():
    s, passes = SC.skeleton(_bin("ones_33x129")[0], return_passes=True)
    assert (int(s.sum()), passes) == (97, 17) and passes > 2 * SC.K                 # more than two launch groups
    assert SC.expected("block_2x2").sum() == 1
    rect = SC.expected("rect_5x9")[0]
    assert rect.sum() == 5 and rect[5, 5:10].all()                                  # the middle row of the rectangle at rows 3 .. 7
    i = np.arange(8)
    d, a = SC.expected("diagonal")[0], SC.expected("anti_diagonal")[0]
    assert _bin("diagonal").sum() == _bin("anti_diagonal").sum() == 15
    assert d.sum() == 8 and d[2 + i, 2 + i].all()
    assert a.sum() == 8 and a[9 - i, 2 + i].all()
    bar = SC.expected("bar_3x8_three_borders")[0]
    assert bar.sum() == 6 and bar[1, 1:7].all()


def test_the_cases_hold_what_they_are_meant_to():
    c = SC.cases()
    H, W = SC.SHAPE
    assert H > SC.TH and W > SC.TW and W % SC.WORD and (W - SC.TW) % SC.WORD and 2 * SC.K <= SC.WORD
    for name in ("cracks", "cracks_2_seams", "batch4"):
        b = c[name][-1 if name != "batch4" else 1] > 0.5
        assert b[0].any() and b[-1].any() and b[:, 0].any() and b[:, -1].any()                     # all four borders
        for sx in range(SC.SEAM_X, b.shape[1], SC.SEAM_X):
            assert b[:, sx - 1].any() and b[:, sx].any()
        assert b[SC.SEAM_Y - 1].any() and b[SC.SEAM_Y].any()
        assert b[SC.SEAM_Y - 1:SC.SEAM_Y + 1, SC.SEAM_X - 1:SC.SEAM_X + 1].all()                   # the corner where four tiles meet
    blob = c["corner_blob"][0] > 0.5
    assert blob[SC.SEAM_Y, SC.SEAM_X] and blob[SC.SEAM_Y].sum() > 2 * (2 * SC.K) and SC.skeleton(blob, return_passes=True)[1] > 3 * SC.K
    assert c["narrow_70x19"].shape[2] < SC.WORD and c["width_33"].shape[2] == SC.WORD + 1 and c["noise_37x70"].shape == (1, 37, 70)
    passes = [SC.skeleton(p > 0.5, return_passes=True)[1] for p in c["batch4"]]
    assert len(set(passes)) == 4 and min(passes) == 1 and max(passes) > 2 * SC.K, passes


@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_invariants(name):
    for img, s in zip(_bin(name), SC.expected(name).astype(bool)):
        assert not (s & ~img).any()                                                 # skeleton is a subset of the input
        assert np.array_equal(SC.skeleton(s), s) and SC.one_pass(s)[1] == 0         # idempotent
        assert SC.components(s) == SC.components(img)                               # 8-connectivity preserved
        assert s.any() == img.any()


@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_the_tiled_form_reaches_the_same_skeleton(name):
    """the kernel's design: K passes per launch on TH x TW tiles with a halo of 2 K, repeated until a launch deletes nothing"""
    for img, s in zip(_bin(name), SC.expected(name).astype(bool)):
        got, groups = SC.tiled_skeleton(img, SC.K, SC.TH, SC.TW)
        assert np.array_equal(got, s)
        assert np.array_equal(SC.tiled(got, SC.K, SC.TH, SC.TW)[0], got)            # further launches change nothing


@pytest.mark.parametrize("k,th,tw", [(1, 32, 64), (3, 32, 64), (4, 32, 64), (3, 7, 5)])
def test_the_tiled_form_at_other_tilings(k, th, tw):
    img = _bin("cracks")[0]
    assert np.array_equal(SC.tiled_skeleton(img, k, th, tw)[0], SC.expected("cracks")[0].astype(bool))
    one = SC.tiled(img, k, th, tw)[0]                                               # one launch = k whole-plane passes
    assert np.array_equal(one, SC.skeleton(img, max_passes=k))


def test_max_passes_is_that_many_hand_applied_passes():
    img = _bin("corner_blob")[0]
    cur = img
    for p in range(1, SC.K + 3):
        cur = SC.sub_iteration(SC.sub_iteration(cur, 0)[0], 1)[0]
        assert np.array_equal(SC.skeleton(img, max_passes=p), cur), p
    small = _bin("rect_5x9")[0]
    assert np.array_equal(SC.skeleton(small, max_passes=50), SC.skeleton(small))    # min(p, passes to convergence)


# ------------------------------------------------------------------------------------------------ scores
def test_score_conventions():
    from csbsr_amd.inference import cldice_scores, summarize_cldice
    from csbsr_amd.utils import estimate_metrics as EM
    assert EM.cldice_scores is cldice_scores and EM.summarize_cldice is summarize_cldice
    c = np.array([[10, 5, 8, 4],         # Tprec 1/2, Tsens 1/2, clDice 1/2
                  [0, 0, 8, 4],          # nothing predicted: Tprec 1
                  [10, 5, 0, 0],         # no ground truth: Tsens 1
                  [0, 0, 0, 0],          # neither: 1, 1, 1
                  [10, 0, 8, 0],         # nothing matches: 0, 0, 0
                  [4, 4, 3, 1]])         # 1, 1/3, 1/2
    tp, ts, cl = cldice_scores(c)
    assert all(a.dtype == np.float64 and a.shape == (6,) for a in (tp, ts, cl))
    assert tp.tolist() == [0.5, 1.0, 0.5, 1.0, 0.0, 1.0] and ts.tolist() == [0.5, 0.5, 1.0, 1.0, 0.0, 1 / 3]
    assert cl[:5].tolist() == [0.5, 2 * 0.5 / 1.5, 2 * 0.5 / 1.5, 1.0, 0.0] and abs(cl[5] - 0.5) <= 2.0 ** -52
    for g, w in zip((tp, ts, cl), SC.scores_naive(c)):
        assert np.array_equal(g, np.array(w))
    s = summarize_cldice(c)
    assert list(s) == ["clDice", "Tprec", "Tsens", "clDice_pooled"] and all(isinstance(v, float) for v in s.values())
    assert s["clDice"] == float(np.mean(cl)) and s["Tprec"] == float(np.mean(tp)) and s["Tsens"] == float(np.mean(ts))
    pooled = SC.scores_naive([c.sum(0)])[2][0]                                      # (34, 14, 27, 9)
    assert s["clDice_pooled"] == pooled and abs(pooled - 2 * (14 / 34) * (9 / 27) / (14 / 34 + 9 / 27)) <= 2.0 ** -52
    assert summarize_cldice(np.zeros((1, 4), np.int64)) == {"clDice": 1.0, "Tprec": 1.0, "Tsens": 1.0, "clDice_pooled": 1.0}


def test_counts_of_the_pair():
    pred, mask, t = SC.pair()
    c = SC.counts(pred, mask, t)
    assert c.dtype == np.int64 and (c[:, 1] <= c[:, 0]).all() and (c[:, 3] <= c[:, 2]).all()
    assert (c[:2] > 0).all() and c[2].tolist()[1:] == [0, 0, 0] and c[2, 0] > 0      # image 2: an empty mask, a predicted blob
    assert c[1, 3] < c[1, 2] and np.isnan(pred).any() and not SC.binarise(pred, t)[np.isnan(pred)].any()
    assert not SC.binarise(pred, t)[pred == np.float32(0.3)].any() and (mask == np.float32(0.5)).any()


def test_csv_writers(tmp_path):
    from csbsr_amd.inference import cldice_scores, mean_width, write_cldice_log, write_crack_stats
    c = np.array([[10, 5, 8, 4], [0, 0, 0, 0], [7, 0, 3, 0]])
    names = ["a.png", "b.png", "c.png"]
    write_cldice_log(str(tmp_path / "cldice_log.csv"), c, names)
    rows = SC.read_csv(str(tmp_path / "cldice_log.csv"))
    assert rows[0] == ["", "skel_pred", "skel_pred_in_gt", "skel_gt", "skel_gt_in_pred", "Tprec", "Tsens", "clDice"] and len(rows) == 4
    assert [r[0] for r in rows[1:]] == names and np.array_equal(np.array([[int(v) for v in r[1:5]] for r in rows[1:]]), c)
    for k, a in enumerate(cldice_scores(c)):
        assert [float(r[5 + k]) for r in rows[1:]] == a.tolist()
    assert (mean_width(12, 5), mean_width(0, 0), mean_width(3, 0)) == (12 / 5, 0.0, 0.0) and isinstance(mean_width(4, 2), float)
    stats = [("a.png", 12, 5, mean_width(12, 5)), ("b.png", 0, 0, 0.0)]
    write_crack_stats(str(tmp_path / "crack_stats.csv"), stats)
    rows = SC.read_csv(str(tmp_path / "crack_stats.csv"))
    assert rows[0] == ["name", "crack_px", "skeleton_px", "mean_width_px"]
    assert [(r[0], int(r[1]), int(r[2]), float(r[3])) for r in rows[1:]] == stats


def test_evaluate_dataset_host_logic_over_cpu_stand_ins(monkeypatch, tmp_path):
    """evaluate_dataset has no CPU path: its device calls are replaced by plain torch stand-ins, centerline_counts by the restatement; the
    accumulation, the keys, the summary and the files are what runs."""
    import eval_io_cases as EC
    from csbsr_amd import inference as I

    def stitch(p, shape, clip, want_f32=True, want_u8=False):
        nH, nW, Cc, ph, pw = [int(v) for v in shape][2:]
        B = p.shape[0] // (nH * nW)
        f = p.view(B, nH, nW, Cc, ph, pw).permute(0, 3, 1, 4, 2, 5).reshape(B, Cc, nH * ph, nW * pw)
        return (f.clamp(0, 1) if clip else f), None

    calls = []

    def cl(seg, masks, threshold):
        calls.append(threshold)
        H, W = seg.shape[-2:]
        return torch.from_numpy(SC.counts(seg.reshape(-1, H, W).numpy(), masks.reshape(-1, H, W).numpy(), threshold).astype(np.int32))

    monkeypatch.setattr(I, "stitch_clip_u8", stitch)
    monkeypatch.setattr(I, "psnr_ssim", lambda a, b: ((a - b).flatten(1).pow(2).mean(1), (a * b).flatten(1).mean(1)))
    monkeypatch.setattr(I, "iou_sweep", lambda seg, m, th, smooth=1e-5: torch.zeros(seg.shape[0], len(th)))
    monkeypatch.setattr(I, "centerline_counts", cl)
    monkeypatch.setattr(I, "_Saver", lambda d, th: os.makedirs(d))
    hr, masks, lr, kernels, names = EC.make_testset(11, 4, 64, 96, 4, zero_mask=3)
    items = [EC.reference_item_numpy(hr[i], masks[i], lr[i], kernels[i], (32, 48), 4, 2) for i in range(4)]
    col = lambda i0, k: torch.from_numpy(np.stack([it[k] for it in items[i0:i0 + 2]]))
    batches = [(col(i0, 0), col(i0, 1), col(i0, 2), col(i0, 3), names[i0:i0 + 2], items[i0][4], items[i0][5]) for i0 in (0, 2)]
    plain = I.evaluate_dataset(EC.stub_model, batches, save_dir=str(tmp_path / "plain"))
    assert calls == [] and "cl_counts" not in plain and os.listdir(tmp_path / "plain") == ["iou_log.csv"]
    out = I.evaluate_dataset(EC.stub_model, batches, cldice_threshold=0.5, save_dir=str(tmp_path / "cl"))
    keys = {"clDice", "Tprec", "Tsens", "clDice_pooled"}
    assert calls == [0.5, 0.5] and set(out) == set(plain) | {"cl_counts"} and set(out["summary"]) == set(plain["summary"]) | keys
    assert out["cl_counts"].dtype == np.int64 and out["cl_counts"].shape == (4, 4) and (out["cl_counts"][3, 2:] == 0).all()
    assert {k: out["summary"][k] for k in keys} == I.summarize_cldice(out["cl_counts"])
    assert {k: out["summary"][k] for k in plain["summary"]} == plain["summary"]
    assert sorted(os.listdir(tmp_path / "cl")) == ["cldice_log.csv", "iou_log.csv"]
    rows = SC.read_csv(str(tmp_path / "cl" / "cldice_log.csv"))
    assert [r[0] for r in rows[1:]] == out["fnames"] and [[int(v) for v in r[1:5]] for r in rows[1:]] == out["cl_counts"].tolist()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_matches_the_header():
    from csbsr_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    ctype = {"const float*": L.vp, "const uint32_t*": L.vp, "uint32_t*": L.vp, "const uint8_t*": L.vp, "uint8_t*": L.vp, "int32_t*": L.vp,
             "csbsr_stream_t": L.vp, "int32_t": L.i32, "float": L.f32}
    nargs = {}
    for name in ENTRIES:
        decl = re.search(r"(int|int32_t)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl, f"{name} is not declared in include/csbsr_hip.h"
        body = decl.group(2).replace("\n", " ").strip()
        args = [] if body == "void" else [ctype[" ".join(a.split()[:-1])] for a in body.split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is L.i32 and sig == args, name
        nargs[name] = len(args)
    assert nargs == {"csbsr_skeleton_max_passes": 0, "csbsr_skeleton_init": 7, "csbsr_skeleton_passes": 8, "csbsr_skeleton_finish": 6,
                     "csbsr_centerline_counts": 10}
    assert "skeleton.hip" in open(os.path.join(ROOT, "csbsr_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "csbsr_amd", "csrc", "skeleton.hip")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (SK_TH|SK_TWW|SK_K) (\d+)", src)}
    assert (consts["SK_TH"], SC.WORD * consts["SK_TWW"], consts["SK_K"]) == (SC.TH, SC.TW, SC.K)     # the cases straddle the kernel's seams


# ------------------------------------------------------------------------------------------------ refusals, before anything runs
def _no_library(monkeypatch):
    from csbsr_amd import _lib as L
    monkeypatch.setattr(L, "load", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(L, "call", lambda *a: pytest.fail("a kernel was launched"))


def test_skeletonize_refuses_bad_arguments(monkeypatch):
    from csbsr_amd.utils.estimate_metrics import centerline_counts, skeletonize
    _no_library(monkeypatch)
    x = torch.zeros(1, 4, 4)
    for bad in (float("nan"), float("inf"), -float("inf"), 1, None, "0.5", True, torch.tensor(0.5)):
        with pytest.raises(ValueError):
            skeletonize(x, threshold=bad)
        with pytest.raises(ValueError):
            centerline_counts(x, x, bad)
    for bad in (-1, -8, 1.5, None, True):
        with pytest.raises(ValueError):
            skeletonize(x, max_passes=bad)
    p = inspect.signature(skeletonize).parameters
    assert p["threshold"].default == 0.5 and p["max_passes"].default == 0


def test_the_drivers_refuse_bad_thresholds_and_default_to_none(monkeypatch):
    from csbsr_amd import inference as I
    _no_library(monkeypatch)
    model = lambda *a, **k: pytest.fail("the model ran")

    class Loader:
        def __iter__(self):
            pytest.fail("the loader was read")

    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf"), 1, "0.5", True):
        with pytest.raises(ValueError):
            I.evaluate_dataset(model, Loader(), cldice_threshold=bad)
        with pytest.raises(ValueError):
            I.evaluate_batch(model, None, None, None, None, None, None, 21, cldice_threshold=bad)
        with pytest.raises(ValueError):
            next(I.predict_dataset(model, Loader(), measure_threshold=bad))
    assert inspect.signature(I.evaluate_dataset).parameters["cldice_threshold"].default is None
    assert inspect.signature(I.evaluate_batch).parameters["cldice_threshold"].default is None
    assert inspect.signature(I.predict_dataset).parameters["measure_threshold"].default is None
    assert "ONE threshold, not the sweep" in I.evaluate_dataset.__doc__               # and the docstring says why
