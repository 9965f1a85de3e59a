"""Host side of the scale-jittered crop (RandomResizedCrop) of the resident loader, no GPU: the ABI declaration, the NumPy restatement of
csbsr_gather_resize_u8 against torch's CPU interpolate and against the fixture recorded from the reference's transforms, the window draw
against torchvision's published get_params, check_windows, and the cfg spelling."""
import os
import re

import numpy as np
import pytest
import torch

import resized_crop_cases as RZ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(40, 52), (31, 45), (24, 32), (50, 33), (37, 64), (29, 41), (44, 36)]


@pytest.fixture(scope="module")
def R():
    from csbsr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "csbsr_amd", "csrc"), "-j8"], check=True)
    from csbsr_amd.data import resident
    return resident


def make_dataset(R, sizes=SIZES, seed=0):
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for H, W in sizes]
    masks = [rng.integers(0, 256, size=(H, W), dtype=np.uint8) for H, W in sizes]
    return R.ResidentDataset(images, masks, device="cpu")


def test_header_and_signatures_name_the_resize():
    from csbsr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    m = re.search(r"\bint\s+csbsr_gather_resize_u8\s*\(([^;]*)\)\s*;", hdr)
    assert m
    res, args = _lib.SIGNATURES["csbsr_gather_resize_u8"]
    assert res is _lib.i32 and len(args) == 11 == len(m.group(1).split(","))
    assert args[8] is _lib.i32                              # the antialias flag, between w and out


# ------------------------------------------------------------------------------------------------------------------- restatement
CASES = [("parity", RZ.CROP), ("odd", RZ.ODD_OUT), ("wide", RZ.WIDE_OUT)]


def _case(name, out):
    if name == "wide":
        images, masks = RZ.wide_inputs()
        return images, masks, RZ.wide_rows()
    images, masks = RZ.parity_inputs()
    return images, masks, RZ.parity_rows_for(*out)


@pytest.mark.parametrize("antialias", [1, 0])
@pytest.mark.parametrize("name,out", CASES)
def test_fp32_restatement_against_torch(name, out, antialias):
    """E = max|fp32 restatement - fp64 restatement| <= 2 * max|torch CPU fp32 - fp64 restatement| + 2^-24, the rule the kernel is held
    to: this checks the restatement (and the rule) where torch runs."""
    images, masks, rows = _case(name, out)
    for arrays in (images, masks):
        r64, e_ref, bound = RZ.tolerance(arrays, rows, *out, antialias)
        e = float(np.abs(RZ.gather_resize_numpy(arrays, rows, *out, antialias, np.float32).astype(np.float64) - r64).max())
        print(f"{name} {out} antialias {antialias} C {arrays[0].ndim == 3 and 3 or 1}: E_np32 {e:.3e}  E_ref {e_ref:.3e}  bound {bound:.3e}")
        assert e <= bound


def test_identity_window_is_the_plain_gather():
    import resident_cases as RC
    images, masks = RZ.parity_inputs()
    h, w = RZ.CROP
    rows7 = np.array([(0, 13, 16, 1, 0, h, w), (4, 0, 7, 0, 1, h, w), (1, 0, 0, 1, 1, h, w)], dtype=np.int32)
    for antialias in (1, 0):
        assert np.array_equal(RZ.gather_resize_numpy(images, rows7, h, w, antialias, np.float32), RC.gather_numpy(images, rows7[:, :5], h, w))
        assert np.array_equal(RZ.gather_resize_torch(masks, rows7, h, w, antialias), RC.gather_numpy(masks, rows7[:, :5], h, w))


def test_fixture_is_reproduced_by_the_restatement():
    g = RZ.load_golden()
    h, w = g["crop"]
    assert (h, w) == RZ.CROP and g["sel"].shape == (12, 7) and os.path.getsize(RZ.GOLDEN) < 200 * 1024
    assert {(int(r[3]), int(r[4])) for r in g["sel"]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for arrays, want in ((g["images"], g["out_image"]), (g["masks"], g["out_mask"])):
        r64, e_ref, bound = RZ.tolerance(arrays, g["sel"], h, w, 1)
        assert float(np.abs(want.astype(np.float64) - r64).max()) <= bound          # the fixture IS torch's CPU result
        e = float(np.abs(RZ.gather_resize_numpy(arrays, g["sel"], h, w, 1, np.float32).astype(np.float64) - r64).max())
        print(f"fixture: E_np32 {e:.3e}  E_ref {e_ref:.3e}")
        assert e <= bound
    m = g["out_mask"]
    assert ((m > 0) & (m < 1)).sum() > 100                  # the mask goes through the bilinear resample: soft


# ------------------------------------------------------------------------------------------------------------------- the draw
def test_draw_windows_follow_get_params(R):
    ds = make_dataset(R)
    scale, ratio = (0.3, 0.9), (0.75, 4 / 3)
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=7, seed=3, resized_crop={"scale": scale, "ratio": ratio}, vflip_p=0.4)
    twin = torch.Generator().manual_seed(3)
    seen = []
    for _ in range(40):
        if ld._perm is None or ld._cursor >= len(ld._perm):
            torch.randperm(len(ds), generator=twin)         # the epoch's permutation comes first
        sel, params = ld.draw()
        sel = sel.numpy()
        assert sel.dtype == np.int32 and sel.shape == (7, 7) and params.shape == (7, 3)
        u = torch.rand(7, 24, generator=twin, dtype=torch.float64).numpy()
        ld.deg.gen = twin
        ld.deg.draw_params(7)                               # the blur draws advance the twin as they advanced the loader
        ld.deg.gen = ld.gen
        for row, ur in zip(sel, u):
            H, W = ds.dims[row[0]]
            y0, x0, hs, ws, took = RZ.get_params(int(H), int(W), scale, ratio, ur[:20].reshape(10, 2), ur[20:22])
            assert tuple(row[[1, 2, 5, 6]]) == (y0, x0, hs, ws) and took
            assert row[3] == (ur[22] < 0.5) and row[4] == (ur[23] < 0.4)
        ds.check_windows(sel, 24, 32)
        seen.append(sel)
    rows = np.concatenate(seen)
    H, W = ds.dims[rows[:, 0]].T.astype(np.float64)
    hs, ws = rows[:, 5].astype(np.float64), rows[:, 6].astype(np.float64)
    assert (rows[:, 1] >= 0).all() and (rows[:, 1] + rows[:, 5] <= H).all() and (rows[:, 2] >= 0).all() and (rows[:, 2] + rows[:, 6] <= W).all()
    # round() moves each side by at most 1/2 from the real sides a, b: the area by at most (a + b) / 2 + 1/4 <= (hs + ws + 1) / 2 + 1/4,
    # and the real aspect a / b lies between (ws - 1/2) / (hs + 1/2) and (ws + 1/2) / (hs - 1/2)
    slack = ((hs + ws + 1) / 2 + 0.25) / (H * W)
    frac = hs * ws / (H * W)
    assert (frac >= scale[0] - slack).all() and (frac <= scale[1] + slack).all()
    assert ((ws + 0.5) / (hs - 0.5) >= ratio[0]).all() and ((ws - 0.5) / (hs + 0.5) <= ratio[1]).all()
    assert frac.min() < 0.4 and frac.max() > 0.8 and (ws / hs).min() < 0.85 and (ws / hs).max() > 1.2      # the ranges are used
    assert rows[:, 3].any() and not rows[:, 3].all() and rows[:, 4].any() and not rows[:, 4].all()


def test_draw_fallback_is_central(R):
    """Images whose aspect lies outside ``ratio`` with scale (1, 1): no try fits, so every window is the central fallback."""
    ds = make_dataset(R, sizes=[(20, 60), (60, 20), (30, 30)])
    ld = R.DeviceTrainLoader(ds, (16, 16), 4, batch_size=3, seed=0, shuffle=False, resized_crop={"scale": (1.0, 1.0), "ratio": (0.5, 2.0)})
    for _ in range(5):
        sel = ld.draw()[0].numpy()
        assert [tuple(r[[0, 1, 2, 5, 6]]) for r in sel] == [(0, 0, 10, 20, 40), (1, 10, 0, 40, 20), (2, 0, 0, 30, 30)]
    # and the restated get_params agrees about the fallback
    assert RZ.get_params(20, 60, (1.0, 1.0), (0.5, 2.0), np.full((10, 2), 0.5), (0.3, 0.3)) == (0, 10, 20, 40, False)
    assert RZ.get_params(60, 20, (1.0, 1.0), (0.5, 2.0), np.full((10, 2), 0.5), (0.3, 0.3)) == (10, 0, 40, 20, False)


def test_draw_is_seeded_and_resumes(R):
    ds = make_dataset(R)
    mk = lambda seed, n=None: R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=3, seed=seed, num_iterations=n, resized_crop={})
    assert mk(1).resized_crop == ((0.5, 1.0), (1.0, 1.0))                  # the reference's class defaults
    a, b = list(mk(11, 9).iter_decisions()), list(mk(11, 9).iter_decisions())
    assert len(a) == 9 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    assert not all(torch.equal(x[0], y[0]) for x, y in zip(a, mk(12, 9).iter_decisions()))
    assert all(x[0].shape[1] == 7 for x in a) and len({tuple(r[5:]) for x in a for r in x[0].tolist()}) > 10
    first = mk(11, 9)
    it = first.iter_decisions()
    head = [next(it) for _ in range(4)]
    second = mk(999, 9)
    second.load_state_dict(first.state_dict())
    tail = list(second.iter_decisions())
    got = head + tail
    assert len(got) == 9 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(got, a))


def test_option_off_draws_as_before(R):
    """resized_crop=None: the [b,5] rows and the generator's advance are those of four uniforms per sample."""
    ds = make_dataset(R)
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=4, seed=5)
    twin = torch.Generator().manual_seed(5)
    idx = ds.indices[torch.randperm(len(ds), generator=twin).numpy()][:4]
    u = torch.rand(4, 4, generator=twin, dtype=torch.float64).numpy()
    sel = ld.draw()[0].numpy()
    assert sel.shape == (4, 5) and (sel[:, 0] == idx).all() and ld.resized_crop is None
    d = ds.dims[idx].astype(np.int64)
    assert (sel[:, 1] == np.minimum((u[:, 0] * (d[:, 0] - 24 + 1)).astype(np.int64), d[:, 0] - 24)).all()
    assert (sel[:, 3] == (u[:, 2] < 0.5)).all()


def test_loader_argument_validation(R):
    ds = make_dataset(R)
    for bad in ({"scale": (0.0, 1.0)}, {"scale": (0.8, 0.5)}, {"ratio": (0.0, 1.0)}, {"ratio": (2.0, 1.0)}, {"scales": (0.5, 1.0)}):
        with pytest.raises(ValueError):
            R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=2, resized_crop=bad)
    small = make_dataset(R, sizes=[(12, 40), (30, 9)])
    with pytest.raises(ValueError):                          # smaller than the crop: refused without the option ...
        R.DeviceTrainLoader(small, (24, 32), 4, batch_size=2)
    ld = R.DeviceTrainLoader(small, (24, 32), 4, batch_size=2, seed=0, resized_crop={"ratio": (0.5, 2.0)})       # ... upsampled with it
    small.check_windows(ld.draw()[0].numpy(), 24, 32)
    with pytest.raises(ValueError):                          # an image whose windows could exceed the kernel's 8x limit
        R.DeviceTrainLoader(make_dataset(R, sizes=[(40, 300)]), (24, 32), 4, batch_size=1, resized_crop={})


# ------------------------------------------------------------------------------------------------------------------- check_windows
def test_check_windows(R):
    ds = make_dataset(R)
    good = np.array([(0, 0, 0, 0, 0, 40, 52), (1, 30, 44, 1, 1, 1, 1), (6, 4, 6, 1, 0, 40, 30)], dtype=np.int32)
    ds.check_windows(good, 24, 32)
    ds.check_windows(good, 5, 7)                             # 40 <= 8 * 5, 52 <= 8 * 7
    def bad(row, h=24, w=32, table=None):
        t = good.copy() if table is None else table
        if row is not None:
            t[1] = row
        with pytest.raises(ValueError):
            ds.check_windows(t, h, w)
    bad((1, 30, 44, 0, 0, 2, 1))                             # leaves the image at the bottom
    bad((1, 0, 40, 0, 0, 5, 6))                              # ... at the right
    bad((1, -1, 0, 0, 0, 5, 6))
    bad((1, 0, 0, 0, 0, 0, 6))                               # hs = 0
    bad((1, 0, 0, 0, 0, 6, -3))
    bad((1, 0, 0, 2, 0, 6, 6))                               # a bad flip
    bad((1, 0, 0, 0, -1, 6, 6))
    bad((7, 0, 0, 0, 0, 6, 6))                               # no such image
    bad(None, h=4, w=32)                                     # 40 > 8 * 4: over the cap in y
    bad(None, h=24, w=6)                                     # 52 > 8 * 6: over the cap in x
    bad(None, table=good[:, :5].copy())                      # the [B][5] table is check_selection's
    bad(None, table=good.astype(np.float32))
    with pytest.raises(ValueError):                          # and the [B][5] contract of check_selection stays
        ds.check_selection(good, 24, 32)


# ------------------------------------------------------------------------------------------------------------------- cfg spelling
def test_cfg_list_spelling(R):
    ds = make_dataset(R)
    entry = ["RandomResizedCrop", [{"scale": (0.5, 1.0), "ratio": (1.0, 1.0)}]]
    aug = [["ConvertFromInts", "None"], ["RandomMirror", "None"], ["ToTensor", "None"], entry]
    with pytest.raises(NotImplementedError):                 # the function itself still refuses it
        R.interpret_augmentation(aug, (24, 32), ds.dims)
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=5, seed=2, augmentation=aug)
    assert ld.resized_crop == ((0.5, 1.0), (1.0, 1.0)) and ld.mirror_p == 0.5
    sel = ld.draw()[0].numpy()
    assert sel.shape == (5, 7) and (sel[:, 5] == sel[:, 6]).all()            # ratio (1, 1): square windows
    ds.check_windows(sel, 24, 32)
    # the same draws as the explicit argument with the default list (whose RandomCrop stands where the entry stood)
    twin = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=5, seed=2, resized_crop={"scale": (0.5, 1.0), "ratio": (1.0, 1.0)})
    assert np.array_equal(twin.draw()[0].numpy(), sel)
    # an explicit argument wins over the list
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=5, seed=2, augmentation=aug, resized_crop={"scale": (0.2, 0.3), "ratio": (2.0, 2.0)})
    assert ld.resized_crop == ((0.2, 0.3), (2.0, 2.0))
    # the ordering rules still hold for the place the entry stands in
    with pytest.raises(NotImplementedError):
        R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=5, augmentation=[["ToTensor", None], entry, ["RandomMirror", None]])
    with pytest.raises(NotImplementedError):
        R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=5, augmentation=[["ToTensor", None], entry, ["RandomCrop", None]])
    # the identity entry stays interpret_augmentation's
    ident = ["RandomResizedCrop", [{"scale": (1.0, 1.0), "ratio": (1.0, 1.0)}]]
    same = make_dataset(R, sizes=[(24, 32)] * 3)
    assert R.DeviceTrainLoader(same, (24, 32), 4, batch_size=2, augmentation=[["ToTensor", None], ident]).resized_crop is None
    assert R.split_resized_crop(aug)[0][-1] == ("RandomCrop", None) and R.split_resized_crop(R.DEFAULT_AUGMENTATION)[1] is None


def test_from_cfg_passes_the_list_through(R):
    from csbsr_amd.config import cfg as base
    cfg = base.clone()
    cfg._merge({"DATASET": {"DATA_AUGMENTATION": [["ConvertFromInts", "None"], ["RandomMirror", "None"], ["ToTensor", "None"],
                                                  ["RandomResizedCrop", [{"scale": [0.6, 0.9], "ratio": [0.8, 1.25]}]]]}})
    ld = R.DeviceTrainLoader.from_cfg(cfg, make_dataset(R), crop=(24, 32), seed=1)
    assert ld.resized_crop == ((0.6, 0.9), (0.8, 1.25)) and ld.draw()[0].shape[1] == 7
