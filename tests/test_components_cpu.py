"""Connected components without a GPU: the kernel's local-then-merge form against the definition on every case of the GPU tests, what the
cases are meant to hold, the skeleton identity the driver rests on, the C ABI, the argument refusals and the crack_instances.csv round trip."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import components_cases as CC
import skeleton_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"csbsr_ccl_tile": 2, "csbsr_ccl_label": 9, "csbsr_component_sums": 7, "csbsr_component_keep": 9}
TH, TW = CC.TH, CC.TW


def _bin(name):
    planes, t = CC.cases()[name]
    return SC.binarise(planes, t)


# ------------------------------------------------------------------------------------------------ the definition on literal patterns
def test_canonical_labels_on_literal_patterns():
    img = np.array([[0, 1, 0, 0, 1],
                    [1, 0, 0, 0, 1],
                    [0, 0, 1, 0, 0],
                    [0, 0, 0, 1, 1]], bool)
    assert CC.canonical_labels(img, 8).tolist() == [[0, 2, 0, 0, 5], [2, 0, 0, 0, 5], [0, 0, 13, 0, 0], [0, 0, 0, 13, 13]]
    assert CC.canonical_labels(img, 4).tolist() == [[0, 2, 0, 0, 5], [6, 0, 0, 0, 5], [0, 0, 13, 0, 0], [0, 0, 0, 19, 19]]
    lab = CC.canonical_labels(img, 8)[None]
    skel = np.zeros((1, 4, 5), np.uint8)
    skel[0, 3, 3] = skel[0, 0, 0] = 7                                               # (0, 0) is background: it counts for no component
    assert CC.table(lab, skel).tolist() == [[0, 2, 2, 0, 0, 0, 1, 1], [0, 5, 2, 0, 0, 4, 1, 4], [0, 13, 3, 1, 2, 2, 3, 4]]
    assert CC.table(lab, None, 3).tolist() == [[0, 13, 3, 0, 2, 2, 3, 4]]
    assert CC.keep(lab, 3)[0].tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 1]]
    assert np.array_equal(CC.keep(lab, 1)[0], img)
    assert CC.cracks_of(CC.table(lab, skel, 3), 5) == [dict(y=2, x=2, area_px=3, length_px=1, mean_width_px=3.0, bbox=(2, 2, 3, 4))]


# ------------------------------------------------------------------------------------------------ the kernel's form
@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("name", sorted(CC.cases()))
def test_the_tiled_form_equals_the_definition(name, connectivity):
    for img, want in zip(_bin(name), CC.expected(name, connectivity)):
        got = CC.tiled_labels(img, connectivity)
        assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_the_local_pass_alone_does_not_join_across_a_seam():
    """the merge matters: without it every seam case differs from the definition"""
    for name in ("corner_diagonal", "u_down", "u_left", "comb_hseam", "serpentine", "noise_0.45"):
        img = _bin(name)[0]
        H, W = img.shape
        local = np.zeros((H, W), np.int32)
        for y0 in range(0, H, TH):
            for x0 in range(0, W, TW):
                t = CC.canonical_labels(img[y0:y0 + TH, x0:x0 + TW], 8)
                local[y0:y0 + TH, x0:x0 + TW] = np.where(t > 0, t + 10 ** 6 * (y0 + x0 + 1), 0)
        assert len(np.unique(local)) > len(np.unique(CC.expected(name)[0])), name


# ------------------------------------------------------------------------------------------------ the inputs
def _n(name, connectivity):
    return int(np.count_nonzero(np.unique(CC.expected(name, connectivity))))


def test_the_cases_hold_what_they_are_meant_to():
    H, W = CC.SHAPE
    assert H > TH and W > TW and W % CC.WORD and (W - TW) % CC.WORD
    c = CC.cases()
    assert c["ones"][0].shape == (1, TH + 6, TW + 5) and _n("ones", 8) == _n("ones", 4) == 1
    assert c["width_33"][0].shape[2] == 33 and c["width_19"][0].shape[2] == 19 and c["1xW_line"][0].shape == (1, 1, W)
    assert _n("zeros", 8) == _n("1x1_clear", 8) == 0 and CC.expected("1x1_set").tolist() == [[[1]]]
    for name in ("corner_diagonal", "corner_anti_diagonal"):                        # one component at 8, two at 4
        assert (_n(name, 8), _n(name, 4)) == (1, 2) and _bin(name).sum() == 2
    for name in ("hseam_diagonals", "vseam_diagonals"):
        assert (_n(name, 8), _n(name, 4)) == (2, 4)
    assert _bin("corner_diagonal")[0][TH - 1, TW - 1] and _bin("corner_diagonal")[0][TH, TW]
    assert _bin("corner_anti_diagonal")[0][TH - 1, TW] and _bin("corner_anti_diagonal")[0][TH, TW - 1]
    for o, far in (("down", np.s_[TH:, :]), ("up", np.s_[:TH, :]), ("right", np.s_[:, TW:]), ("left", np.s_[:, :TW])):
        img = _bin(f"u_{o}")[0]
        near = img.copy()
        near[far] = False                                                           # without the far side the arms are two components
        assert _n(f"u_{o}", 8) == _n(f"u_{o}", 4) == 1 and SC.components(near) == 2, o
    for name, near in (("comb_hseam", np.s_[:TH, :]), ("comb_vseam", np.s_[:, :TW])):
        img = _bin(name)[0]
        assert _n(name, 8) == _n(name, 4) == 1 and SC.components(img[near]) >= 16
    s = _bin("serpentine")[0]
    assert s.shape == (70, 133) and s.sum() == 4690 and _n("serpentine", 4) == 1
    sp = _bin("spiral")[0]
    assert _n("spiral", 4) == _n("spiral", 8) == 1 and H * W // 3 < sp.sum() < 0.6 * H * W and SC.components(~sp) == 1
    assert _n("checkerboard", 8) == 1 and _n("checkerboard", 4) == H * W // 2 == _bin("checkerboard").sum()
    for d in CC.DENSITIES:
        for conn in (8, 4):
            lab = CC.expected(f"noise_{d}", conn)[0]
            assert _n(f"noise_{d}", conn) >= 10 and min(CC.crosses_seams(lab)) >= 1, (d, conn)
    if (TH, TW) == (64, 128):
        assert [_n(f"noise_{d}", 8) for d in CC.DENSITIES] == [658, 464, 87, 10]
        assert [_n(f"noise_{d}", 4) for d in CC.DENSITIES] == [1142, 1192, 876, 297]
    assert c["cracks_2_vseams"][0].shape == (1, TH + 3, 2 * TW + 7) and c["cracks_2_hseams"][0].shape == (1, 2 * TH + 3, TW + 7)
    for name in ("cracks_2_vseams", "cracks_2_hseams"):
        assert _n(name, 8) >= 4 and min(CC.crosses_seams(CC.expected(name)[0])) >= 1
    b = CC.expected("batch5")
    assert b.shape[0] == 5 and np.array_equal(b[1], b[4]) and b[2].max() == 0
    assert np.count_nonzero(np.unique(b[0])) == 1 and np.count_nonzero(np.unique(b[1])) >= 4 and np.count_nonzero(np.unique(b[3])) >= 10
    pred, t = c["pair_special_values"]
    assert np.isnan(pred).any() and np.isinf(pred).any() and (pred == np.float32(t)).any()


# ------------------------------------------------------------------------------------------------ the identity the driver rests on
@pytest.mark.parametrize("name,plane", [("noise_37x70", 0), ("batch4", 3), ("batch4", 1), ("cracks", 0)])
def test_the_skeleton_of_the_kept_components_is_the_kept_part_of_the_skeleton(name, plane):
    """two 8-connected components never share a 3 x 3 neighbourhood and the deletion rule reads no more: one thinning serves them all"""
    img = SC.cases()[name][plane] > 0.5
    whole = SC.skeleton(img)
    lab = CC.canonical_labels(img, 8)[None]
    for min_px in (1, 5, 20):
        k = CC.keep(lab, min_px)[0].astype(bool)
        assert np.array_equal(SC.skeleton(k), whole & k), (name, min_px)
    assert not CC.keep(lab, 10 ** 6).any()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_matches_the_header():
    from csbsr_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    ctype = {"const float*": L.vp, "const uint8_t*": L.vp, "uint8_t*": L.vp, "const int32_t*": L.vp, "csbsr_stream_t": L.vp, "int32_t": L.i32,
             "float": L.f32}
    for name, n in ENTRIES.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl, f"{name} is not declared in include/csbsr_hip.h"
        args = [" ".join(a.split()[:-1]) for a in decl.group(1).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is L.i32 and len(sig) == len(args) == n, name
        if name != "csbsr_ccl_tile":
            assert sig == [L.vp if a == "int32_t*" else ctype[a] for a in args], name
    assert "components.hip" in open(os.path.join(ROOT, "csbsr_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "csbsr_amd", "csrc", "components.hip")).read()
    consts = {k: int(v) for k, v in re.findall(r"#define (CC_TH|CC_TWW|CC_MAX_SIDE|CC_ACC) (\d+)", src)}
    assert (consts["CC_TH"], CC.WORD * consts["CC_TWW"]) == (TH, TW)               # the cases straddle the kernel's seams
    from csbsr_amd.utils import estimate_metrics as M
    assert consts["CC_MAX_SIDE"] == 8192 and consts["CC_ACC"] == M.CC_ACC and M.TABLE_COLUMNS == CC.COLUMNS
    assert "Coherence" in src and "Termination" in src                              # the header comment carries both arguments


# ------------------------------------------------------------------------------------------------ refusals, before anything runs
def _no_library(monkeypatch):
    from csbsr_amd import _lib as L
    monkeypatch.setattr(L, "load", lambda: pytest.fail("the library was loaded"))
    monkeypatch.setattr(L, "call", lambda *a: pytest.fail("a kernel was launched"))


def test_the_host_api_refuses_bad_arguments(monkeypatch):
    from csbsr_amd.utils.estimate_metrics import component_table, keep_components, label_components
    _no_library(monkeypatch)
    x = torch.zeros(1, 4, 4)
    lab = torch.zeros(1, 4, 4, dtype=torch.int32)
    for bad in (float("nan"), float("inf"), 1, None, "0.5", True):
        with pytest.raises(ValueError):
            label_components(x, threshold=bad)
    for bad in (0, 1, 6, 8.0, "8", None, True):
        with pytest.raises(ValueError):
            label_components(x, connectivity=bad)
    for bad in (0, -1, 1.0, 2.5, "3", None, True, False):
        with pytest.raises(ValueError):
            component_table(lab, min_px=bad)
        with pytest.raises(ValueError):
            keep_components(lab, bad)
    p = inspect.signature(label_components).parameters
    assert p["threshold"].default == 0.5 and p["connectivity"].default == 8
    p = inspect.signature(component_table).parameters
    assert p["skeleton"].default is None and p["min_px"].default == 1


def test_predict_dataset_refuses_a_bad_min_crack_px_before_the_model_runs(monkeypatch):
    from csbsr_amd import inference as I
    _no_library(monkeypatch)
    model = lambda *a, **k: pytest.fail("the model ran")

    class Loader:
        def __iter__(self):
            pytest.fail("the loader was read")

    with pytest.raises(ValueError):                                                  # nothing to filter without a measurement
        next(I.predict_dataset(model, Loader(), min_crack_px=5))
    for bad in (0, -3, 5.0, 2.5, "5", True, False):
        with pytest.raises(ValueError):
            next(I.predict_dataset(model, Loader(), measure_threshold=0.4, min_crack_px=bad))
    with pytest.raises(ValueError):
        next(I.predict_dataset(model, Loader(), measure_threshold=1.0, min_crack_px=5))
    assert inspect.signature(I.predict_dataset).parameters["min_crack_px"].default is None


# ------------------------------------------------------------------------------------------------ crack_instances.csv
def test_crack_instances_round_trip(tmp_path):
    from csbsr_amd import inference as I
    lab = CC.expected("cracks_2_vseams")
    skel = CC.expected_skeleton("cracks_2_vseams")
    W = lab.shape[2]
    rows = CC.table(lab, skel, 5)
    assert len(rows) >= 3
    cracks = I.crack_instances(rows.tolist(), W)
    assert cracks == CC.cracks_of(rows, W) and all(type(c["mean_width_px"]) is float and type(c["area_px"]) is int for c in cracks)
    assert [(c["y"], c["x"]) for c in cracks] == sorted((c["y"], c["x"]) for c in cracks)           # raster order of the first pixel
    assert I.crack_instances([[0, 7, 4, 0, 0, 6, 1, 7]], 10) == [dict(y=0, x=6, area_px=4, length_px=0, mean_width_px=0.0, bbox=(0, 6, 1, 7))]
    images = [("a.png", cracks), ("empty.png", []), ("b.png", cracks[:1])]
    path = str(tmp_path / "crack_instances.csv")
    I.write_crack_instances(path, images)
    raw = SC.read_csv(path)
    assert raw[0] == ["name", "crack", "y", "x", "area_px", "length_px", "mean_width_px", "y0", "x0", "y1", "x1"] == I.INSTANCE_COLUMNS
    assert len(raw) == 1 + len(cracks) + 1 and [r[1] for r in raw[1:]] == [str(j) for j in range(len(cracks))] + ["0"]
    assert I.read_crack_instances(path) == [("a.png", cracks), ("b.png", cracks[:1])]                # an image without cracks has no row
