"""csrc/components.hip and its drivers on the device: every result is an integer and is asked for exactly, against the NumPy / SciPy
restatement of tests/components_cases.py (whose own properties tests/test_components_cpu.py holds).

Through the C ABI every input sits inside an allocation filled with +inf -- a read outside the planes would set pixels -- and every output
and scratch array inside a sentinel-filled allocation whose margins are checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import components_cases as CC
import skeleton_cases as SC

pytestmark = pytest.mark.gpu

PAD = 64
ISENT, BSENT = 0x5A5A5A5A, 0x5A
DEV = torch.device("cuda", 0)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _inp(x, fill, dtype=torch.float32):
    x = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape(-1)
    buf = torch.full((x.numel() + 2 * PAD,), fill, dtype=dtype, device=DEV)
    buf[PAD:PAD + x.numel()] = x.to(DEV)
    return buf, buf[PAD:PAD + x.numel()]


def _out(n, dtype=torch.int32):
    buf = torch.full((n + 2 * PAD,), ISENT if dtype == torch.int32 else BSENT, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _margins_intact(*wholes):
    for w in wholes:
        sent = ISENT if w.dtype == torch.int32 else BSENT
        assert bool((w[:PAD] == sent).all()) and bool((w[-PAD:] == sent).all()), "a write outside an output"


def device_labels(planes, threshold, connectivity, fill=float("inf")):
    """int32 [N, H, W] of csbsr_ccl_label through the C ABI"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = planes.shape
    _, x = _inp(planes, fill)
    (ww, work), (wl, labels) = _out(N * H * W), _out(N * H * W)
    L.call("csbsr_ccl_label", _ptr(x), threshold, N, H, W, connectivity, _ptr(work), _ptr(labels), _stream())
    torch.cuda.synchronize()
    _margins_intact(ww, wl)
    return labels.cpu().numpy().reshape(N, H, W)


def device_sums_and_keep(labels, skeleton, min_px):
    """(acc int32 [N, 5, H W] with the sentinel where nothing was written, keep uint8 [N, H, W], kept labels int32 [N, H, W]) through the C ABI;
    the labels and the skeleton sit between label-like / skeleton-like values"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = labels.shape
    _, lab = _inp(labels, 1, torch.int32)
    sk = None if skeleton is None else _inp(skeleton, 1, torch.uint8)[1]
    (wa, acc), (wk, keep), (wo, kept) = _out(N * 5 * H * W), _out(N * H * W, torch.uint8), _out(N * H * W)
    L.call("csbsr_component_sums", _ptr(lab), None if sk is None else _ptr(sk), N, H, W, _ptr(acc), _stream())
    L.call("csbsr_component_keep", _ptr(lab), _ptr(acc), N, H, W, min_px, _ptr(keep), _ptr(kept), _stream())
    torch.cuda.synchronize()
    _margins_intact(wa, wk, wo)
    return acc.cpu().numpy().reshape(N, 5, H * W), keep.cpu().numpy().reshape(N, H, W), kept.cpu().numpy().reshape(N, H, W)


def test_the_tile_is_the_one_the_cases_straddle():
    from csbsr_amd import _lib as L
    lib = L.load()
    th, tw = C.c_int32(0), C.c_int32(0)
    assert lib.csbsr_ccl_tile(C.byref(th), C.byref(tw)) == 0 and (th.value, tw.value) == (CC.TH, CC.TW)
    assert lib.csbsr_ccl_tile(None, C.byref(tw)) != 0 and lib.csbsr_ccl_tile(C.byref(th), None) != 0


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize("connectivity", [8, 4])
@pytest.mark.parametrize("name", sorted(CC.cases()))
def test_labels_equal_the_definition(name, connectivity):
    planes, t = CC.cases()[name]
    got = device_labels(planes, t, connectivity)
    want = CC.expected(name, connectivity)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]


@pytest.mark.parametrize("connectivity,density", [(8, 0.41), (4, 0.59)])
def test_labels_of_a_plane_of_many_tiles(connectivity, density):
    """1000 x 1100 just under the percolation threshold: 16 x 9 tiles, components that wind through many of them, more workgroups than the
    device runs at once in the merge's neighbourhood of every seam"""
    img = np.random.default_rng(41).random((1, 1000, 1100)) < density
    want = CC.canonical_labels(img[0], connectivity)
    area = np.bincount(want.ravel())[1:]
    assert area.max() > 10 * CC.TH * CC.TW and np.count_nonzero(area) > 1000               # one component larger than ten tiles, and many small ones
    got = device_labels(SC._f32(img), 0.5, connectivity)
    assert np.array_equal(got[0], want), np.argwhere(got[0] != want)[:5]


@pytest.mark.parametrize("name", ["batch5", "noise_0.45", "cracks_2_hseams", "u_up"])
def test_planes_with_ones_around_them(name):
    """the neighbours in the batch and the allocation around it are all set: a plane's labels do not change"""
    planes, t = CC.cases()[name]
    full = np.ones((1,) + planes.shape[1:], np.float32)
    for connectivity in (8, 4):
        got = device_labels(np.concatenate([full, planes, full]), t, connectivity, fill=1.0)
        assert np.array_equal(got[1:-1], CC.expected(name, connectivity))
        assert (got[0] == 1).all() and (got[-1] == 1).all()


def test_label_components_surface():
    from csbsr_amd.utils.estimate_metrics import label_components
    pred, t = CC.cases()["pair_special_values"]
    want = CC.expected("pair_special_values")
    p = torch.from_numpy(pred).to(DEV)
    out = label_components(p, t)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == pred.shape and np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(label_components(p[:, None], t).cpu().numpy(), want)                     # [B, 1, H, W] -> [B, H, W]
    assert np.array_equal(label_components(torch.from_numpy(pred), np.float32(t), connectivity=4).cpu().numpy(),
                          CC.labels_of(pred, np.float32(t), 4))
    planes, _ = CC.cases()["batch5"]
    assert np.array_equal(label_components(torch.from_numpy(planes).to(DEV)).cpu().numpy(), CC.expected("batch5"))   # the defaults: 0.5, 8
    with pytest.raises(ValueError):
        label_components(p, connectivity=6)
    with pytest.raises(ValueError):
        label_components(p, threshold=float("nan"))


def test_two_calls_return_equal_tensors():
    from csbsr_amd.utils.estimate_metrics import component_table, keep_components, label_components
    planes, _ = CC.cases()["batch5"]
    x = torch.from_numpy(planes).to(DEV)
    sk = torch.from_numpy(CC.expected_skeleton("batch5")).to(DEV)
    a, b = label_components(x), label_components(x)
    assert torch.equal(a, b)
    assert torch.equal(component_table(a, sk), component_table(b, sk)) and torch.equal(keep_components(a, 5), keep_components(b, 5))


# ------------------------------------------------------------------------------------------------ table and filter
TABLE_CASES = [("noise_0.3", 8), ("noise_0.6", 4), ("checkerboard", 4), ("checkerboard", 8), ("serpentine", 8), ("cracks_2_vseams", 8),
               ("batch5", 8), ("pair_special_values", 8), ("ones", 4), ("zeros", 8), ("1x1_set", 8)]


@pytest.mark.parametrize("name,connectivity", TABLE_CASES)
def test_table_and_keep_equal_the_restatement(name, connectivity):
    from csbsr_amd.utils.estimate_metrics import component_table, keep_components
    lab_np, skel_np = CC.expected(name, connectivity), CC.expected_skeleton(name)
    N, H, W = lab_np.shape
    lab, skel = torch.from_numpy(lab_np).to(DEV), torch.from_numpy(skel_np).to(DEV)
    region = lab_np > 0
    for min_px in (1, 5, 20):
        for s_np, s in ((skel_np, skel), (None, None)):
            got = component_table(lab, s, min_px)
            want = CC.table(lab_np, s_np, min_px)
            assert got.is_cuda and got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 8
            assert np.array_equal(got.cpu().numpy(), want), (min_px, s is None)
        k = keep_components(lab, min_px)
        assert k.is_cuda and k.dtype == torch.uint8 and tuple(k.shape) == (N, H, W) and np.array_equal(k.cpu().numpy(), CC.keep(lab_np, min_px))
        # the C ABI: margins, the kept labels, and the accumulators written at the roots only
        acc, k_abi, kept = device_sums_and_keep(lab_np, skel_np, min_px)
        assert np.array_equal(k_abi, CC.keep(lab_np, min_px)) and np.array_equal(kept, np.where(k_abi != 0, lab_np, 0))
        roots = lab_np.reshape(N, H * W) == np.arange(1, H * W + 1)
        assert (acc[~np.broadcast_to(roots[:, None], acc.shape)] == ISENT).all()
        full = CC.table(lab_np, skel_np)
        assert np.array_equal(acc.transpose(0, 2, 1)[roots], full[:, [2, 3, 5, 6, 7]])
    assert np.array_equal(keep_components(lab, 1).cpu().numpy().astype(bool), region)               # min_px = 1 keeps the binarised plane
    if name == "checkerboard" and connectivity == 4:
        assert component_table(lab).shape[0] == H * W // 2
    if name == "serpentine":
        assert component_table(lab).cpu().tolist() == [[0, 1, 4690, 0, 0, 0, H - 1, W - 1]]


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    L.load()
    x = torch.ones(64, device=DEV)
    work, lab, kept = (torch.full((64,), ISENT, dtype=torch.int32, device=DEV) for _ in range(3))
    acc = torch.full((5 * 64,), ISENT, dtype=torch.int32, device=DEV)
    sk, keep = torch.ones(64, dtype=torch.uint8, device=DEV), torch.full((64,), BSENT, dtype=torch.uint8, device=DEV)
    st = _stream()
    good = dict(N=1, H=8, W=8)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(H=-8), dict(W=-8), dict(H=8193), dict(W=8193), dict(N=65536)):
        d = {**good, **bad}
        dims = (d["N"], d["H"], d["W"])
        for call in (("csbsr_ccl_label", _ptr(x), 0.5, *dims, 8, _ptr(work), _ptr(lab), st),
                     ("csbsr_component_sums", _ptr(lab), _ptr(sk), *dims, _ptr(acc), st),
                     ("csbsr_component_keep", _ptr(lab), _ptr(acc), *dims, 1, _ptr(keep), _ptr(kept), st)):
            with pytest.raises(L.CsbsrHipError):
                L.call(*call)
    for connectivity in (0, 1, 6, 9, -8):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_ccl_label", _ptr(x), 0.5, 1, 8, 8, connectivity, _ptr(work), _ptr(lab), st)
    for th in (float("nan"), float("inf")):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_ccl_label", _ptr(x), th, 1, 8, 8, 8, _ptr(work), _ptr(lab), st)
    for min_px in (0, -1):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_component_keep", _ptr(lab), _ptr(acc), 1, 8, 8, min_px, _ptr(keep), _ptr(kept), st)
    for call in (("csbsr_ccl_label", None, 0.5, 1, 8, 8, 8, _ptr(work), _ptr(lab), st),
                 ("csbsr_ccl_label", _ptr(x), 0.5, 1, 8, 8, 8, None, _ptr(lab), st),
                 ("csbsr_ccl_label", _ptr(x), 0.5, 1, 8, 8, 8, _ptr(work), None, st),
                 ("csbsr_ccl_label", _ptr(x), 0.5, 1, 8, 8, 8, _ptr(lab), _ptr(lab), st),          # the scratch is another array
                 ("csbsr_component_sums", None, _ptr(sk), 1, 8, 8, _ptr(acc), st),
                 ("csbsr_component_sums", _ptr(lab), _ptr(sk), 1, 8, 8, None, st),
                 ("csbsr_component_keep", None, _ptr(acc), 1, 8, 8, 1, _ptr(keep), _ptr(kept), st),
                 ("csbsr_component_keep", _ptr(lab), None, 1, 8, 8, 1, _ptr(keep), _ptr(kept), st),
                 ("csbsr_component_keep", _ptr(lab), _ptr(acc), 1, 8, 8, 1, None, _ptr(kept), st)):
        with pytest.raises(L.CsbsrHipError):
            L.call(*call)
    torch.cuda.synchronize()
    for t in (work, lab, kept, acc):                                                # nothing ran: no output was written
        assert bool((t == ISENT).all())
    assert bool((keep == BSENT).all())


# ------------------------------------------------------------------------------------------------ the driver
def test_predict_dataset_with_min_crack_px(tmp_path):
    """test_predict_dataset_with_measure_threshold's two images (stitched maps of 64 x 96 and 84 x 68), measured crack by crack"""
    from PIL import Image
    import eval_io_cases as EC
    import predict_cases as PC
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd.inference import INSTANCE_COLUMNS, predict_dataset, read_crack_instances
    images = PC.make_images(PC.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t, k = 0.4, 5
    plain_keys = {"name", "sr_u8", "map_u8", "map_f32", "kernels"}
    measure_keys = plain_keys | {"crack_px", "skeleton_px", "mean_width_px"}
    for batch_patches in (16, 4):                                                   # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        assert len(list(ld)) == (1 if batch_patches == 16 else 2)
        want = PC.host_chain(ld, images, EC.stub_model, torch.from_numpy, EC.thresholds32()[EC.SAVE_IDX])
        save = tmp_path / str(batch_patches)
        got = list(predict_dataset(EC.stub_model, ld, save_dir=str(save), measure_threshold=t, min_crack_px=k))
        one = list(predict_dataset(EC.stub_model, ld, measure_threshold=t, min_crack_px=1))
        measured = list(predict_dataset(EC.stub_model, ld, measure_threshold=t))
        plain = list(predict_dataset(EC.stub_model, ld))
        stats, inst = [], []
        for g, o, m, p, w in zip(got, one, measured, plain, want):
            assert set(p) == plain_keys and set(m) == measure_keys
            assert set(g) == set(o) == measure_keys | {"removed_px", "n_cracks", "labels", "cracks"}
            assert np.array_equal(g["map_f32"].cpu().numpy().view(np.uint32), w["map_f32"].view(np.uint32))
            assert torch.equal(g["map_f32"], p["map_f32"]) and torch.equal(g["sr_u8"], p["sr_u8"]) and torch.equal(g["map_u8"], p["map_u8"])
            # the NumPy chain
            H, W = w["map_f32"].shape
            region = SC.binarise(w["map_f32"], t)
            lab = CC.canonical_labels(region, 8)[None]
            kept = CC.keep(lab, k)[0].astype(bool)
            skel = SC.skeleton(region) & kept
            assert np.array_equal(skel, SC.skeleton(kept))                          # the identity: one thinning serves the filtered plane
            rows = CC.table(lab, skel[None].astype(np.uint8), k)
            assert len(rows) >= 2 and len(CC.table(lab)) - len(rows) >= 1, "every image keeps two components and loses one"
            for key in ("crack_px", "skeleton_px", "removed_px", "n_cracks"):
                assert type(g[key]) is int, key
            assert (g["crack_px"], g["skeleton_px"], g["removed_px"], g["n_cracks"]) == (int(kept.sum()), int(skel.sum()),
                                                                                        int(region.sum() - kept.sum()), len(rows))
            assert g["removed_px"] > 0 and type(g["mean_width_px"]) is float and g["mean_width_px"] == int(kept.sum()) / int(skel.sum())
            assert g["labels"].is_cuda and g["labels"].dtype == torch.int32 and tuple(g["labels"].shape) == (H, W)
            assert np.array_equal(g["labels"].cpu().numpy(), np.where(kept, lab[0], 0))
            assert g["cracks"] == CC.cracks_of(rows, W) and sum(c["area_px"] for c in g["cracks"]) == g["crack_px"]
            assert sum(c["length_px"] for c in g["cracks"]) == g["skeleton_px"]
            assert all(g["labels"][c["y"], c["x"]].item() == c["y"] * W + c["x"] + 1 for c in g["cracks"])
            im = Image.open(save / "skeletons" / g["name"])
            assert im.mode == "L" and np.array_equal(np.array(im), skel.astype(np.uint8) * 255), g["name"]
            stats.append((g["name"], g["crack_px"], g["skeleton_px"], g["mean_width_px"]))
            inst.append((g["name"], g["cracks"]))
            # min_crack_px = 1 removes nothing and measures what the call without it measures
            assert o["removed_px"] == 0 and (o["crack_px"], o["skeleton_px"], o["mean_width_px"]) == (m["crack_px"], m["skeleton_px"],
                                                                                                    m["mean_width_px"])
            assert o["n_cracks"] == len(CC.table(lab)) and np.array_equal(o["labels"].cpu().numpy(), lab[0])
            assert (m["crack_px"], m["skeleton_px"]) == (int(region.sum()), int(SC.skeleton(region).sum()))
        assert sorted(os.listdir(save)) == ["crack_instances.csv", "crack_stats.csv", "images", "kernels", "kernels_origin", "masks", "skeletons"]
        assert sorted(os.listdir(save / "skeletons")) == names
        rows = SC.read_csv(str(save / "crack_stats.csv"))
        assert rows[0] == ["name", "crack_px", "skeleton_px", "mean_width_px"]
        assert [(r[0], int(r[1]), int(r[2]), float(r[3])) for r in rows[1:]] == stats
        assert SC.read_csv(str(save / "crack_instances.csv"))[0] == INSTANCE_COLUMNS
        assert read_crack_instances(str(save / "crack_instances.csv")) == inst
    # without the new option: today's folders and files
    for _ in predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / "measured"), measure_threshold=t):
        pass
    assert sorted(os.listdir(tmp_path / "measured")) == ["crack_stats.csv", "images", "kernels", "kernels_origin", "masks", "skeletons"]
    for _ in predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / "plain")):
        pass
    assert sorted(os.listdir(tmp_path / "plain")) == ["images", "kernels", "kernels_origin", "masks"]
    # an empty region: no cracks
    g = next(predict_dataset(lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs)), ld, measure_threshold=t,
                             min_crack_px=k))
    assert (g["crack_px"], g["skeleton_px"], g["mean_width_px"], g["removed_px"], g["n_cracks"], g["cracks"]) == (0, 0, 0.0, 0, 0, [])
    assert int(g["labels"].abs().sum()) == 0
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(min_crack_px=k), dict(measure_threshold=t, min_crack_px=0), dict(measure_threshold=t, min_crack_px=True),
                   dict(measure_threshold=t, min_crack_px=5.0)):
        with pytest.raises(ValueError):
            next(predict_dataset(model, ld, **kwargs))
