"""csrc/width.hip and its drivers on the device: every result is an integer and is asked for exactly, against the SciPy restatement of
tests/width_cases.py (whose own properties tests/test_width_cpu.py holds).

Through the C ABI the planes sit inside an allocation filled with 0.0 -- 0.0 is background, so a read outside a plane would shorten a
distance --, with more than the largest halo (128 rows and 128 columns) of it on either side; the skeleton and the labels sit between
skeleton-like and label-like values, and every output inside a sentinel-filled allocation whose margins are checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import components_cases as CC
import skeleton_cases as SC
import width_cases as WC

pytestmark = pytest.mark.gpu

PAD = 64
ISENT = 0x5A5A5A5A
DEV = torch.device("cuda", 0)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _inp(x, fill, dtype=torch.float32, pad=PAD):
    x = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape(-1)
    buf = torch.full((x.numel() + 2 * pad,), fill, dtype=dtype, device=DEV)
    buf[pad:pad + x.numel()] = x.to(DEV)
    return buf, buf[pad:pad + x.numel()]


def _out(n):
    buf = torch.full((n + 2 * PAD,), ISENT, dtype=torch.int32, device=DEV)
    return buf, buf[PAD:PAD + n]


def _margins_intact(*wholes):
    for w in wholes:
        assert bool((w[:PAD] == ISENT).all()) and bool((w[-PAD:] == ISENT).all()), "a write outside an output"


def device_width(planes, skeleton, threshold, r, fill=0.0):
    """(d2 int32 [N, H, W], hist int32 [N, r^2 + 2]) of csbsr_skeleton_width through the C ABI"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = planes.shape
    _, x = _inp(planes, fill, pad=(WC.MAX_RADIUS + 2) * (W + 2))                    # background further than any halo reaches
    _, sk = _inp(skeleton, 1, torch.uint8)
    (wd, d2), (wh, hist) = _out(N * H * W), _out(N * (r * r + 2))
    L.call("csbsr_skeleton_width", _ptr(x), threshold, _ptr(sk), N, H, W, r, _ptr(d2), _ptr(hist), _stream())
    torch.cuda.synchronize()
    _margins_intact(wd, wh)
    return d2.cpu().numpy().reshape(N, H, W), hist.cpu().numpy().reshape(N, r * r + 2)


def device_wacc(labels, d2):
    """int32 [N, 2, H W] of csbsr_component_width through the C ABI, the sentinel where nothing was written"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = labels.shape
    _, lab = _inp(labels, 1, torch.int32)
    _, d = _inp(d2, 7, torch.int32)
    ww, wacc = _out(N * 2 * H * W)
    L.call("csbsr_component_width", _ptr(lab), _ptr(d), N, H, W, _ptr(wacc), _stream())
    torch.cuda.synchronize()
    _margins_intact(ww)
    return wacc.cpu().numpy().reshape(N, 2, H * W)


def _wacc_equals_the_restatement(wacc, labels, d2):
    N, H, W = labels.shape
    roots = labels.reshape(N, H * W) == np.arange(1, H * W + 1)
    assert (wacc[~np.broadcast_to(roots[:, None], wacc.shape)] == ISENT).all(), "a slot that is no root was written"
    rows = WC.width_rows(labels, d2)
    assert len(rows) == roots.sum()
    first = np.where(rows[:, 3] >= 0, rows[:, 3] * W + rows[:, 4], -1)
    assert np.array_equal(wacc.transpose(0, 2, 1)[roots], np.stack([rows[:, 2], first], 1))


def test_the_tile_and_the_radius_are_the_ones_the_cases_straddle():
    from csbsr_amd import _lib as L
    lib = L.load()
    th, tw = C.c_int32(0), C.c_int32(0)
    assert lib.csbsr_width_tile(C.byref(th), C.byref(tw)) == 0 and (th.value, tw.value) == (WC.TH, WC.TW)
    assert lib.csbsr_width_tile(None, C.byref(tw)) != 0 and lib.csbsr_width_tile(C.byref(th), None) != 0
    assert lib.csbsr_width_max_radius() == WC.MAX_RADIUS == 128


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name,r", WC.case_radii())
def test_d2_and_hist_equal_the_definition(name, r):
    planes, sk, t, _ = WC.cases()[name]
    got_d2, got_hist = device_width(planes, sk, t, r)
    want_d2, want_hist = WC.expected(name, r)
    assert got_d2.dtype == np.int32 and np.array_equal(got_d2, want_d2), np.argwhere(got_d2 != want_d2)[:5]
    assert np.array_equal(got_hist, want_hist), np.argwhere(got_hist != want_hist)[:5]
    assert (got_hist.sum(axis=1) == (sk != 0).sum(axis=(1, 2))).all()


@pytest.mark.parametrize("kind", ["h", "v"])
def test_straight_bars_have_their_width_on_the_centerline(kind):
    planes, sk, t, _ = WC.cases()[f"bars_{kind}"]
    d2, _ = device_width(planes, sk, t, 64)
    for w, d, s in zip(WC.BAR_WIDTHS, d2, sk):
        assert {WC.width(int(v)) for v in d[s != 0]} == {float(w if w % 2 else w - 1)}, w


@pytest.mark.parametrize("name,r", WC.case_radii())
def test_component_width_equals_the_restatement(name, r):
    labels, (d2, _) = WC.expected_labels(name), WC.expected(name, r)
    _wacc_equals_the_restatement(device_wacc(labels, d2), labels, d2)


def test_component_width_of_any_d2():
    """d2 need not come from a skeleton: every pixel carries a value, ties in every component"""
    labels = WC.expected_labels("noise_0.6")
    d2 = np.random.default_rng(8).integers(0, 4, size=labels.shape).astype(np.int32)
    _wacc_equals_the_restatement(device_wacc(labels, d2), labels, d2)


def test_a_plane_of_ones_between_planes_of_zeros_stays_saturated():
    H, W = WC.SHAPE
    planes = np.stack([np.zeros((H, W), np.float32), np.ones((H, W), np.float32), np.zeros((H, W), np.float32)])
    sk = np.ones((3, H, W), np.uint8)
    for r in (1, 64, 128):
        d2, hist = device_width(planes, sk, 0.5, r, fill=0.0)
        assert (d2[1] == r * r + 1).all() and (d2[0] == 0).all() and (d2[2] == 0).all()
        assert hist[1, -1] == H * W and hist[1].sum() == H * W and hist[0, 0] == H * W and hist[2, 0] == H * W


def test_a_plane_of_many_tiles():
    """1000 x 1100: 16 x 9 tiles, cracks of mixed widths through all of them"""
    region, sk = WC.many_tiles()
    want = np.where(sk != 0, WC.d2_of(region, 64), 0)
    assert want.max() >= 64 and (want > 0).sum() > 5000
    got, hist = device_width(SC._f32(region)[None], sk[None], 0.5, 64)
    assert np.array_equal(got[0], want), np.argwhere(got[0] != want)[:5]
    assert np.array_equal(hist[0], np.bincount(want[sk != 0], minlength=64 * 64 + 2))


# ------------------------------------------------------------------------------------------------ the Python surface
def test_skeleton_width_surface():
    from csbsr_amd.utils.estimate_metrics import skeleton_width
    pred, sk, t, _ = WC.cases()["pair_special_values"]
    N, H, W = pred.shape
    want_d2, want_hist = WC.expected("pair_special_values", 33)
    p, s = torch.from_numpy(pred).to(DEV), torch.from_numpy(sk).to(DEV)
    d2, hist = skeleton_width(p, s, t, 33)
    assert d2.is_cuda and d2.dtype == torch.int32 and tuple(d2.shape) == (N, H, W) and np.array_equal(d2.cpu().numpy(), want_d2)
    assert hist.is_cuda and hist.dtype == torch.int32 and tuple(hist.shape) == (N, 33 * 33 + 2) and np.array_equal(hist.cpu().numpy(), want_hist)
    for a, b in ((p[:, None], s), (p[:, None], s[:, None]), (torch.from_numpy(pred), torch.from_numpy(sk)), (p, torch.from_numpy(sk))):
        d2b, histb = skeleton_width(a, b, np.float32(t), np.int64(33))              # [N, 1, H, W]; CPU tensors
        assert d2b.is_cuda and tuple(d2b.shape) == (N, H, W) and torch.equal(d2b, d2) and torch.equal(histb, hist)
    planes, sk5, _, _ = WC.cases()["batch5"]
    d2, hist = skeleton_width(torch.from_numpy(planes).to(DEV), torch.from_numpy(sk5).to(DEV))       # the defaults: 0.5, 64
    assert np.array_equal(d2.cpu().numpy(), WC.expected("batch5", 64)[0]) and np.array_equal(hist.cpu().numpy(), WC.expected("batch5", 64)[1])
    for bad in (dict(skeleton=s[:, :, :-1]), dict(skeleton=s[:-1]), dict(skeleton=s.transpose(1, 2)), dict(skeleton=s.to(torch.int32)),
                dict(threshold=float("nan")), dict(threshold=1), dict(max_radius=0), dict(max_radius=129), dict(max_radius=True),
                dict(max_radius=64.0)):
        with pytest.raises(ValueError):
            skeleton_width(**{**dict(planes=p, skeleton=s, threshold=t, max_radius=33), **bad})


def test_two_calls_return_equal_tensors():
    from csbsr_amd.utils.estimate_metrics import component_width_table, label_components, skeleton_width, skeletonize
    planes, _, _, _ = WC.cases()["batch5"]
    x = torch.from_numpy(planes).to(DEV)
    sk, lab = skeletonize(x), label_components(x)
    assert np.array_equal(sk.cpu().numpy(), WC.cases()["batch5"][1])
    (a, ha), (b, hb) = skeleton_width(x, sk, 0.5, 128), skeleton_width(x, sk, 0.5, 128)
    assert torch.equal(a, b) and torch.equal(ha, hb)
    assert torch.equal(component_width_table(lab, a), component_width_table(lab, b))


@pytest.mark.parametrize("name", ["batch5", "noise_0.3", "noise_0.6", "cracks", "zeros", "ones", "1x1_set", "pair_special_values"])
def test_component_width_table_aligns_with_component_table(name):
    from csbsr_amd.utils.estimate_metrics import component_table, component_width_table
    lab_np, (d2_np, _) = WC.expected_labels(name), WC.expected(name, 5)
    lab, d2 = torch.from_numpy(lab_np).to(DEV), torch.from_numpy(d2_np).to(DEV)
    for min_px in (1, 5, 20):
        got = component_width_table(lab, d2, min_px)
        assert got.is_cuda and got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 5
        assert np.array_equal(got.cpu().numpy(), WC.width_rows(lab_np, d2_np, min_px)), min_px
        assert torch.equal(got[:, :2], component_table(lab, None, min_px)[:, :2])
    assert torch.equal(component_width_table(lab, d2), component_width_table(lab, d2, 1))
    with pytest.raises(ValueError):
        component_width_table(lab, d2, 0)
    with pytest.raises(ValueError):
        component_width_table(lab, d2[:, :-1])


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    L.load()
    x = torch.ones(64, device=DEV)
    sk = torch.ones(64, dtype=torch.uint8, device=DEV)
    lab = torch.ones(64, dtype=torch.int32, device=DEV)
    d2, wacc, hist = (torch.full((n,), ISENT, dtype=torch.int32, device=DEV) for n in (64, 2 * 64, 128 * 128 + 2))
    st = _stream()
    good = dict(N=1, H=8, W=8)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(H=-8), dict(W=-8), dict(H=8193), dict(W=8193), dict(N=65536)):
        d = {**good, **bad}
        dims = (d["N"], d["H"], d["W"])
        for call in (("csbsr_skeleton_width", _ptr(x), 0.5, _ptr(sk), *dims, 4, _ptr(d2), _ptr(hist), st),
                     ("csbsr_component_width", _ptr(lab), _ptr(d2), *dims, _ptr(wacc), st)):
            with pytest.raises(L.CsbsrHipError):
                L.call(*call)
    for r in (0, -1, 129):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_skeleton_width", _ptr(x), 0.5, _ptr(sk), 1, 8, 8, r, _ptr(d2), _ptr(hist), st)
    for th in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_skeleton_width", _ptr(x), th, _ptr(sk), 1, 8, 8, 4, _ptr(d2), _ptr(hist), st)
    for call in (("csbsr_skeleton_width", None, 0.5, _ptr(sk), 1, 8, 8, 4, _ptr(d2), _ptr(hist), st),
                 ("csbsr_skeleton_width", _ptr(x), 0.5, None, 1, 8, 8, 4, _ptr(d2), _ptr(hist), st),
                 ("csbsr_skeleton_width", _ptr(x), 0.5, _ptr(sk), 1, 8, 8, 4, None, _ptr(hist), st),
                 ("csbsr_skeleton_width", _ptr(x), 0.5, _ptr(sk), 1, 8, 8, 4, _ptr(d2), None, st),
                 ("csbsr_component_width", None, _ptr(d2), 1, 8, 8, _ptr(wacc), st),
                 ("csbsr_component_width", _ptr(lab), None, 1, 8, 8, _ptr(wacc), st),
                 ("csbsr_component_width", _ptr(lab), _ptr(d2), 1, 8, 8, None, st)):
        with pytest.raises(L.CsbsrHipError):
            L.call(*call)
    lib = L.load()
    assert lib.csbsr_width_tile(None, None) != 0
    torch.cuda.synchronize()
    for t in (d2, wacc, hist):                                                      # nothing ran: no output was written, no histogram cleared
        assert bool((t == ISENT).all())


# ------------------------------------------------------------------------------------------------ the driver
WIDTH_KEYS = {"max_width_px", "median_width_px", "p95_width_px", "centerline_width_px", "saturated_px", "widest", "width_hist", "width_d2"}


def _check_width_keys(g, d2, skel, r):
    """the new keys of one yielded dict against d2 int32 [H, W] (0 off the skeleton) of the NumPy chain"""
    H, W = d2.shape
    want = WC.summary(d2[skel], r)
    for key in ("max_width_px", "median_width_px", "p95_width_px", "centerline_width_px"):
        assert type(g[key]) is float, key
    assert (g["max_width_px"], g["median_width_px"], g["p95_width_px"], g["saturated_px"]) == (want["max_width_px"], want["median_width_px"],
                                                                                              want["p95_width_px"], want["saturated_px"])
    assert g["centerline_width_px"] == pytest.approx(want["centerline_width_px"], rel=1e-12, abs=0)   # an fp64 mean summed in another order
    assert type(g["saturated_px"]) is int
    assert g["widest"] == (divmod(int(np.argmax(d2)), W) if d2.max() > 0 else None)                   # np.argmax: the first maximum
    assert isinstance(g["width_hist"], np.ndarray) and g["width_hist"].dtype == np.int64 and g["width_hist"].shape == (r * r + 2,)
    assert np.array_equal(g["width_hist"], np.bincount(d2[skel], minlength=r * r + 2))
    assert g["width_d2"].is_cuda and g["width_d2"].dtype == torch.int32 and np.array_equal(g["width_d2"].cpu().numpy(), d2)


def test_predict_dataset_with_width_radius(tmp_path):
    """test_predict_dataset_with_min_crack_px's two images (stitched maps of 64 x 96 and 84 x 68), with the local width"""
    import eval_io_cases as EC
    import predict_cases as PC
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd import inference as I
    predict_dataset = I.predict_dataset
    images = PC.make_images(PC.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t, k, r = 0.4, 5, 64
    measure_keys = {"name", "sr_u8", "map_u8", "map_f32", "kernels", "crack_px", "skeleton_px", "mean_width_px"}
    crack_keys = measure_keys | {"removed_px", "n_cracks", "labels", "cracks"}
    for batch_patches in (16, 4):                                                   # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        want = PC.host_chain(ld, images, EC.stub_model, torch.from_numpy, EC.thresholds32()[EC.SAVE_IDX])
        save, save_w = tmp_path / f"{batch_patches}", tmp_path / f"{batch_patches}_w"
        got = list(predict_dataset(EC.stub_model, ld, save_dir=str(save), measure_threshold=t, min_crack_px=k, width_radius=r))
        whole = list(predict_dataset(EC.stub_model, ld, save_dir=str(save_w), measure_threshold=t, width_radius=2))
        cracks_only = list(predict_dataset(EC.stub_model, ld, measure_threshold=t, min_crack_px=k))
        measured = list(predict_dataset(EC.stub_model, ld, measure_threshold=t))
        widths, inst = [], []
        for g, a, c, m, w in zip(got, whole, cracks_only, measured, want):
            assert set(m) == measure_keys and set(c) == crack_keys                  # without the option: today's keys
            assert set(g) == crack_keys | WIDTH_KEYS and set(a) == measure_keys | WIDTH_KEYS
            H, W = w["map_f32"].shape
            region = SC.binarise(w["map_f32"], t)
            lab = CC.canonical_labels(region, 8)[None]
            kept = CC.keep(lab, k)[0].astype(bool)
            skel = SC.skeleton(region) & kept
            # the kept cracks, measured against the whole region: the same distances as against the kept pixels alone
            d2 = np.where(skel, WC.d2_of(region, r), 0).astype(np.int32)
            assert np.array_equal(d2, np.where(skel, WC.d2_of(kept, r), 0)) and skel.sum() > 0
            _check_width_keys(g, d2, skel, r)
            rows = WC.width_rows(lab, d2[None], k)
            assert len(rows) == len(g["cracks"]) == len(c["cracks"]) >= 2
            for crack, plain, (_, label, m2, y, x) in zip(g["cracks"], c["cracks"], rows.tolist()):
                assert set(crack) == set(plain) | {"max_width_px", "widest"} and {q: crack[q] for q in plain} == plain
                assert (crack["y"] * W + crack["x"] + 1, crack["max_width_px"], crack["widest"]) == (label, WC.width(m2), (y, x) if m2 > 0 else None)
                assert type(crack["max_width_px"]) is float
            assert max(crack["max_width_px"] for crack in g["cracks"]) == g["max_width_px"]
            assert g["widest"] in [crack["widest"] for crack in g["cracks"]]
            # the whole skeleton at a radius that saturates
            skel_all = SC.skeleton(region)
            d2_all = np.where(skel_all, WC.d2_of(region, 2), 0).astype(np.int32)
            _check_width_keys(a, d2_all, skel_all, 2)
            # nothing else changes with the option
            for key in ("map_f32", "sr_u8", "map_u8"):
                assert torch.equal(g[key], m[key]) and torch.equal(a[key], m[key]), key
            assert (g["crack_px"], g["skeleton_px"], g["mean_width_px"]) == (c["crack_px"], c["skeleton_px"], c["mean_width_px"])
            assert (a["crack_px"], a["skeleton_px"], a["mean_width_px"]) == (m["crack_px"], m["skeleton_px"], m["mean_width_px"])
            assert [crack["area_px"] for crack in g["cracks"]] == [crack["area_px"] for crack in c["cracks"]]
            assert torch.equal(g["labels"], c["labels"])
            widths.append((g["name"], dict(centerline_px=int(skel.sum()), **{q: g[q] for q in ("saturated_px", "centerline_width_px", "median_width_px",
                                                                                              "p95_width_px", "max_width_px", "widest")})))
            inst.append((g["name"], [dict(max_width_px=crack["max_width_px"], widest=crack["widest"]) for crack in g["cracks"]]))
        assert any(a["saturated_px"] > 0 for a in whole), "radius 2 saturates somewhere"
        assert sorted(os.listdir(save)) == ["crack_instance_widths.csv", "crack_instances.csv", "crack_stats.csv", "crack_widths.csv", "images",
                                            "kernels", "kernels_origin", "masks", "skeletons"]
        assert sorted(os.listdir(save_w)) == ["crack_stats.csv", "crack_widths.csv", "images", "kernels", "kernels_origin", "masks", "skeletons"]
        assert SC.read_csv(str(save / "crack_widths.csv"))[0] == I.WIDTH_COLUMNS
        assert I.read_crack_widths(str(save / "crack_widths.csv")) == widths
        assert SC.read_csv(str(save / "crack_instance_widths.csv"))[0] == I.INSTANCE_WIDTH_COLUMNS
        assert I.read_crack_instance_widths(str(save / "crack_instance_widths.csv")) == inst
        assert [n for n, _ in I.read_crack_instances(str(save / "crack_instances.csv"))] == names      # the same numbering
        assert [len(cr) for _, cr in I.read_crack_instances(str(save / "crack_instances.csv"))] == [len(cr) for _, cr in inst]
    # without the new option: today's folders and files
    for _ in predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / "cracks"), measure_threshold=t, min_crack_px=k):
        pass
    assert sorted(os.listdir(tmp_path / "cracks")) == ["crack_instances.csv", "crack_stats.csv", "images", "kernels", "kernels_origin", "masks",
                                                       "skeletons"]
    for _ in predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / "measured"), measure_threshold=t, width_radius=None):
        pass
    assert sorted(os.listdir(tmp_path / "measured")) == ["crack_stats.csv", "images", "kernels", "kernels_origin", "masks", "skeletons"]
    for _ in predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / "plain")):
        pass
    assert sorted(os.listdir(tmp_path / "plain")) == ["images", "kernels", "kernels_origin", "masks"]
    # an all-zero map
    zero = lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs))
    for kwargs in (dict(), dict(min_crack_px=k)):
        g = next(predict_dataset(zero, ld, measure_threshold=t, width_radius=r, **kwargs))
        assert (g["max_width_px"], g["median_width_px"], g["p95_width_px"], g["centerline_width_px"], g["saturated_px"], g["widest"]) == (
            0.0, 0.0, 0.0, 0.0, 0, None)
        assert g["width_hist"].shape == (r * r + 2,) and not g["width_hist"].any() and int(g["width_d2"].abs().sum()) == 0
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(width_radius=r), dict(min_crack_px=k, width_radius=r), dict(measure_threshold=t, width_radius=0),
                   dict(measure_threshold=t, width_radius=129), dict(measure_threshold=t, width_radius=True),
                   dict(measure_threshold=t, width_radius=64.0), dict(measure_threshold=t, width_radius=-1),
                   dict(measure_threshold=t, min_crack_px=k, width_radius="64")):
        with pytest.raises(ValueError):
            next(predict_dataset(model, ld, **kwargs))
