"""csrc/topology.hip and its drivers on the device: every result is an integer and is asked for exactly, against the NumPy restatement of
tests/topology_cases.py (whose own properties tests/test_topology_cpu.py holds).

Through the C ABI the skeleton sits inside an allocation filled with 1 -- a set pixel, so a read outside a plane would add a neighbour or a
link --, the labels between label-like values, and every output inside a sentinel-filled allocation whose margins are checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import components_cases as CC
import skeleton_cases as SC
import topology_cases as TC

pytestmark = pytest.mark.gpu

PAD = 64
ISENT = 0x5A5A5A5A
BSENT = 0x5A
DEV = torch.device("cuda", 0)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _inp(x, fill, dtype, pad):
    x = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape(-1)
    buf = torch.full((x.numel() + 2 * pad,), fill, dtype=dtype, device=DEV)
    buf[pad:pad + x.numel()] = x.to(DEV)
    return buf, buf[pad:pad + x.numel()]


def _out(n, dtype=torch.int32):
    sent = ISENT if dtype == torch.int32 else BSENT
    buf = torch.full((n + 2 * PAD,), sent, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _margins_intact(*wholes):
    for w in wholes:
        sent = ISENT if w.dtype == torch.int32 else BSENT
        assert bool((w[:PAD] == sent).all()) and bool((w[-PAD:] == sent).all()), "a write outside an output"


def device_topology(planes):
    """(topo uint8 [N, H, W], counts int32 [N, 10]) of csbsr_skeleton_topology through the C ABI"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = planes.shape
    _, sk = _inp(planes, 1, torch.uint8, 2 * (W + 2))                                # set pixels before the first and behind the last plane
    (wt, topo), (wc, counts) = _out(N * H * W, torch.uint8), _out(N * 10)
    L.call("csbsr_skeleton_topology", _ptr(sk), N, H, W, _ptr(topo), _ptr(counts), _stream())
    torch.cuda.synchronize()
    _margins_intact(wt, wc)
    return topo.cpu().numpy().reshape(N, H, W), counts.cpu().numpy().reshape(N, 10)


def device_tacc(labels, topo, jlabels):
    """int32 [N, 9, H W] of csbsr_component_topology through the C ABI, the sentinel where nothing was written"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = labels.shape
    _, lab = _inp(labels, 1, torch.int32, PAD)
    _, t = _inp(topo, 0xFF, torch.uint8, PAD)
    jl = None if jlabels is None else _inp(jlabels, 1, torch.int32, PAD)[1]
    wa, tacc = _out(N * 9 * H * W)
    L.call("csbsr_component_topology", _ptr(lab), _ptr(t), None if jl is None else _ptr(jl), N, H, W, _ptr(tacc), _stream())
    torch.cuda.synchronize()
    _margins_intact(wa)
    return tacc.cpu().numpy().reshape(N, 9, H * W)


def _junction_labels(topo):
    return np.stack([CC.canonical_labels((t & 7) == TC.JUNCTION) for t in topo])


def _tacc_equals_the_restatement(tacc, labels, topo, with_junctions=True):
    N, H, W = labels.shape
    roots = labels.reshape(N, H * W) == np.arange(1, H * W + 1)
    assert (tacc[~np.broadcast_to(roots[:, None], tacc.shape)] == ISENT).all(), "a slot that is no root was written"
    rows = TC.topology_rows(labels, topo)
    assert len(rows) == roots.sum()
    want = rows[:, 2:].copy()
    if not with_junctions:
        want[:, 8] = 0
    assert np.array_equal(tacc.transpose(0, 2, 1)[roots], want)


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", list(TC.cases()))
def test_topo_and_counts_equal_the_restatement(name):
    planes = TC.cases()[name]
    got_topo, got_counts = device_topology(planes)
    want_topo, want_counts = TC.expected(name)
    assert got_topo.dtype == np.uint8 and np.array_equal(got_topo, want_topo), np.argwhere(got_topo != want_topo)[:5]
    assert got_counts.dtype == np.int32 and np.array_equal(got_counts, want_counts), (got_counts, want_counts)
    assert (got_counts[:, 0] == (planes != 0).sum(axis=(1, 2))).all()


@pytest.mark.parametrize("name", list(TC.HAND))
def test_hand_shapes_have_their_hand_derived_counts_on_the_device(name):
    plane, want = TC.hand(name), TC.HAND[name][1]
    _, counts = device_topology(plane[None])
    got = dict(zip(TC.COLUMNS, (int(k) for k in counts[0])))
    got["loops"] = SC.components(plane) - TC.euler(counts[0])
    got["length"] = TC.length(got["h"], got["v"], got["d_se"], got["d_sw"])
    assert {k: got[k] for k in want} == want


@pytest.mark.parametrize("h,w", TC.SHAPES + (TC.SHAPE,))
def test_all_ones_have_closed_forms_on_the_device(h, w):
    _, counts = device_topology(np.ones((2, h, w), np.uint8))
    for c in counts:
        assert c.tolist() == [h * w] + c[1:5].tolist() + [h * (w - 1), (h - 1) * w, 0, 0, (h - 1) * (w - 1)] and TC.euler(c) == 1


@pytest.mark.parametrize("name", ["noise_0.05", "noise_0.3", "noise_0.6", "noise_0.95", "cracks", "borders", "seams", "framed_batch", "two_and_one"])
def test_loops_from_the_device_counts_equal_the_flood_fill(name):
    planes = TC.cases()[name]
    _, counts = device_topology(planes)
    for plane, c in zip(planes, counts):
        assert SC.components(plane) - TC.euler(c) == TC.holes(plane)


def test_a_plane_of_many_tiles():
    """520 x 700: 9 x 6 tiles, noise at three densities side by side and an empty band, so that empty and full tiles alternate"""
    rng = np.random.default_rng(12)
    plane = np.zeros((520, 700), np.uint8)
    for k, d in enumerate((0.1, 0.5, 0.9)):
        plane[:, 200 * k:200 * k + 150] = rng.random((520, 150)) < d
    plane[128:192] = 0
    got_topo, got_counts = device_topology(plane[None])
    want = TC.topo_of(plane)
    assert np.array_equal(got_topo[0], want) and np.array_equal(got_counts[0], TC.counts_of(want))


def component_cases():
    """name -> (labels int32 [N, H, W], topo uint8 [N, H, W]): the labels of a region with the topo of its skeleton, and the labels of a
    plane with its own topo"""
    out = {}
    regions = np.stack([TC.crack_region(s) for s in TC.CRACK_SEEDS])
    out["cracks"] = (np.stack([CC.canonical_labels(r) for r in regions]), TC.expected("cracks")[0])
    region, _ = TC.two_and_one()
    out["two_and_one"] = (CC.canonical_labels(region)[None], TC.expected("two_and_one")[0])
    for name in ("noise_0.3", "noise_0.6", "noise_0.05", "seams", "borders", "framed_batch", "ones", "zeros", "noise_5x7", "ones_1x1"):
        out[name] = (np.stack([CC.canonical_labels(p != 0) for p in TC.cases()[name]]), TC.expected(name)[0])
    return out


def test_two_cracks_in_one_tile_and_one_across_four():
    labels, topo = component_cases()["two_and_one"]
    present = sorted(set(labels.ravel().tolist()) - {0})
    assert len(present) == 3
    tiles = [{(y // TC.TH, x // TC.TW) for y, x in np.argwhere(labels[0] == lab)} for lab in present]
    assert sorted(len(t) for t in tiles) == [1, 1, 4] and tiles[0] == tiles[1] == {(0, 0)}
    rows = TC.topology_rows(labels, topo)
    assert (rows[:, 2] >= 2).all() and rows[:, 8].sum() == 0 and rows[2, 10] >= 1   # ends everywhere, no quads, the branch's junction


@pytest.mark.parametrize("name", list(component_cases()))
def test_component_topology_equals_the_restatement(name):
    labels, topo = component_cases()[name]
    _tacc_equals_the_restatement(device_tacc(labels, topo, _junction_labels(topo)), labels, topo)


def test_component_topology_without_junction_labels():
    labels, topo = component_cases()["cracks"]
    _tacc_equals_the_restatement(device_tacc(labels, topo, None), labels, topo, with_junctions=False)


def test_component_topology_of_any_topo():
    """topo need not come from a skeleton: every byte value, in every component"""
    labels = component_cases()["noise_0.6"][0]
    topo = np.random.default_rng(8).integers(0, 256, size=labels.shape).astype(np.uint8)
    _tacc_equals_the_restatement(device_tacc(labels, topo, _junction_labels(topo)), labels, topo)


# ------------------------------------------------------------------------------------------------ the Python surface
def test_skeleton_topology_surface():
    from csbsr_amd.utils.estimate_metrics import skeleton_topology
    planes = TC.cases()["cracks"]
    N, H, W = planes.shape
    want_topo, want_counts = TC.expected("cracks")
    s = torch.from_numpy(planes).to(DEV)
    topo, counts = skeleton_topology(s)
    assert topo.is_cuda and topo.dtype == torch.uint8 and tuple(topo.shape) == (N, H, W) and np.array_equal(topo.cpu().numpy(), want_topo)
    assert counts.is_cuda and counts.dtype == torch.int32 and tuple(counts.shape) == (N, 10) and np.array_equal(counts.cpu().numpy(), want_counts)
    for a in (s[:, None], torch.from_numpy(planes), s * 255, s[0]):                 # [N, 1, H, W]; a CPU tensor; any non-zero byte; one plane
        tb, cb = skeleton_topology(a)
        n = 1 if a.dim() == 2 else N
        assert tb.is_cuda and tuple(tb.shape) == (n, H, W) and torch.equal(tb, topo[:n]) and torch.equal(cb, counts[:n])
    wide = s.repeat(1, 1, 2)[:, :, 1:W + 1]                                         # a view that is not contiguous
    assert np.array_equal(skeleton_topology(wide)[0].cpu().numpy(), TC.topology_of(wide.cpu().numpy())[0])
    for bad in (s.to(torch.int32), s.to(torch.float32), planes, s[0, 0]):
        with pytest.raises(ValueError):
            skeleton_topology(bad)


def test_two_calls_return_equal_tensors():
    from csbsr_amd.utils.estimate_metrics import component_topology_table, label_components, skeleton_topology
    for name in ("noise_0.6", "cracks", "framed_batch"):
        s = torch.from_numpy(TC.cases()[name]).to(DEV)
        (a, ca), (b, cb) = skeleton_topology(s), skeleton_topology(s)
        assert torch.equal(a, b) and torch.equal(ca, cb)
        lab = label_components(s.to(torch.float32), 0.5)
        assert torch.equal(component_topology_table(lab, a), component_topology_table(lab, b))


@pytest.mark.parametrize("name", list(component_cases()))
def test_component_topology_table_aligns_with_component_table(name):
    from csbsr_amd.utils.estimate_metrics import component_table, component_topology_table
    lab_np, topo_np = component_cases()[name]
    lab, topo = torch.from_numpy(lab_np).to(DEV), torch.from_numpy(topo_np).to(DEV)
    for min_px in (1, 5, 20):
        got = component_topology_table(lab, topo, min_px)
        assert got.is_cuda and got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == 11
        assert np.array_equal(got.cpu().numpy(), TC.topology_rows(lab_np, topo_np, min_px)), min_px
        assert torch.equal(got[:, :2], component_table(lab, None, min_px)[:, :2])
    assert torch.equal(component_topology_table(lab, topo), component_topology_table(lab, topo, 1))
    with pytest.raises(ValueError):
        component_topology_table(lab, topo, 0)
    with pytest.raises(ValueError):
        component_topology_table(lab, topo[:, :-1])
    with pytest.raises(ValueError):
        component_topology_table(lab, topo.to(torch.int32))


def test_the_device_labels_give_the_loops_and_junctions_of_the_restatement():
    """the chain predict_dataset runs: components and junction clusters counted on the device, loops from the counts"""
    from csbsr_amd.utils.estimate_metrics import _count_roots, _junction_labels as device_junction_labels, label_components, skeleton_topology
    from csbsr_amd.utils.estimate_metrics import summarize_topology
    for name in ("cracks", "noise_0.3", "borders", "seams"):
        planes = TC.cases()[name]
        s = torch.from_numpy(planes).to(DEV)
        topo, counts = skeleton_topology(s)
        comps = _count_roots(label_components(s.to(torch.float32), 0.5)).cpu().tolist()
        juncs = _count_roots(device_junction_labels(topo)).cpu().tolist()
        for plane, c, nc, nj in zip(planes, counts.cpu().numpy(), comps, juncs):
            got, want = summarize_topology(c, nc, nj), TC.summary(plane)
            assert {k: got[k] for k in want} == want and got["loops"] == TC.holes(plane) and nc == SC.components(plane)


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    L.load()
    sk = torch.ones(64, dtype=torch.uint8, device=DEV)
    topo = torch.full((64,), BSENT, dtype=torch.uint8, device=DEV)
    lab = torch.ones(64, dtype=torch.int32, device=DEV)
    counts, tacc = (torch.full((n,), ISENT, dtype=torch.int32, device=DEV) for n in (10, 9 * 64))
    st = _stream()
    good = dict(N=1, H=8, W=8)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(H=-8), dict(W=-8), dict(H=8193), dict(W=8193), dict(N=65536)):
        d = {**good, **bad}
        dims = (d["N"], d["H"], d["W"])
        for call in (("csbsr_skeleton_topology", _ptr(sk), *dims, _ptr(topo), _ptr(counts), st),
                     ("csbsr_component_topology", _ptr(lab), _ptr(topo), _ptr(lab), *dims, _ptr(tacc), st),
                     ("csbsr_component_topology", _ptr(lab), _ptr(topo), None, *dims, _ptr(tacc), st)):
            with pytest.raises(L.CsbsrHipError):
                L.call(*call)
    for call in (("csbsr_skeleton_topology", None, 1, 8, 8, _ptr(topo), _ptr(counts), st),
                 ("csbsr_skeleton_topology", _ptr(sk), 1, 8, 8, None, _ptr(counts), st),
                 ("csbsr_skeleton_topology", _ptr(sk), 1, 8, 8, _ptr(topo), None, st),
                 ("csbsr_skeleton_topology", _ptr(topo), 1, 8, 8, _ptr(topo), _ptr(counts), st),        # in place
                 ("csbsr_component_topology", None, _ptr(topo), None, 1, 8, 8, _ptr(tacc), st),
                 ("csbsr_component_topology", _ptr(lab), None, None, 1, 8, 8, _ptr(tacc), st),
                 ("csbsr_component_topology", _ptr(lab), _ptr(topo), None, 1, 8, 8, None, st)):
        with pytest.raises(L.CsbsrHipError):
            L.call(*call)
    torch.cuda.synchronize()
    assert bool((topo == BSENT).all())                                               # nothing ran: no output was written, no count cleared
    for t in (counts, tacc):
        assert bool((t == ISENT).all())


# ------------------------------------------------------------------------------------------------ the driver
TOPOLOGY_KEYS = {"endpoints", "junctions", "junction_px", "isolated_px", "loops", "links", "length_geodesic_px", "orientation",
                 "mean_width_geodesic_px", "topology_map"}
CRACK_TOPOLOGY_KEYS = {"endpoints", "junctions", "loops", "links", "length_geodesic_px", "orientation"}


def _check_topology_keys(g, skel, crack_px):
    """the new keys of one yielded dict against the skeleton bool [H, W] of the NumPy chain"""
    want = TC.summary(skel)
    assert {k: g[k] for k in want} == want
    for key in ("endpoints", "junctions", "junction_px", "isolated_px", "loops"):
        assert type(g[key]) is int, key
    assert type(g["length_geodesic_px"]) is float and type(g["mean_width_geodesic_px"]) is float
    assert type(g["links"]) is tuple and type(g["orientation"]) is tuple and all(type(k) is int for k in g["links"])
    assert g["loops"] == TC.holes(skel)
    assert g["mean_width_geodesic_px"] == (crack_px / want["length_geodesic_px"] if want["length_geodesic_px"] else 0.0)
    assert g["topology_map"].is_cuda and g["topology_map"].dtype == torch.uint8 and np.array_equal(g["topology_map"].cpu().numpy(), TC.topo_of(skel))
    return {k: g[k] for k in TOPOLOGY_KEYS - {"topology_map"}}


def _same(a, b):
    """two yielded dicts hold the same keys and the same values"""
    assert set(a) == set(b)
    for key in a:
        if torch.is_tensor(a[key]):
            assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key
        else:
            assert type(a[key]) is type(b[key]) and a[key] == b[key], key


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as fh:
                out[os.path.relpath(os.path.join(d, n), root)] = fh.read()
    return out


def test_predict_dataset_with_topology(tmp_path):
    """test_predict_dataset_with_min_crack_px's two images (stitched maps of 64 x 96 and 84 x 68), with the topology of the skeleton"""
    import eval_io_cases as EC
    import predict_cases as PC
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd import inference as I
    predict_dataset = I.predict_dataset
    images = PC.make_images(PC.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t, k = 0.4, 5
    measure_keys = {"name", "sr_u8", "map_u8", "map_f32", "kernels", "crack_px", "skeleton_px", "mean_width_px"}
    crack_keys = measure_keys | {"removed_px", "n_cracks", "labels", "cracks"}
    for batch_patches in (16, 4):                                                   # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        want = PC.host_chain(ld, images, EC.stub_model, torch.from_numpy, EC.thresholds32()[EC.SAVE_IDX])
        save, save_w = tmp_path / f"{batch_patches}", tmp_path / f"{batch_patches}_w"
        got = list(predict_dataset(EC.stub_model, ld, save_dir=str(save), measure_threshold=t, min_crack_px=k, topology=True))
        whole = list(predict_dataset(EC.stub_model, ld, save_dir=str(save_w), measure_threshold=t, topology=True))
        both = list(predict_dataset(EC.stub_model, ld, measure_threshold=t, min_crack_px=k, width_radius=64, topology=True))
        cracks_only = list(predict_dataset(EC.stub_model, ld, measure_threshold=t, min_crack_px=k))
        measured = list(predict_dataset(EC.stub_model, ld, measure_threshold=t))
        tops, inst = [], []
        for g, a, b, c, m, w in zip(got, whole, both, cracks_only, measured, want):
            assert set(m) == measure_keys and set(c) == crack_keys                  # without the option: today's keys
            assert set(g) == crack_keys | TOPOLOGY_KEYS and set(a) == measure_keys | TOPOLOGY_KEYS
            H, W = w["map_f32"].shape
            region = SC.binarise(w["map_f32"], t)
            lab = CC.canonical_labels(region, 8)[None]
            kept = CC.keep(lab, k)[0].astype(bool)
            skel_all = SC.skeleton(region)
            skel = skel_all & kept
            assert skel.sum() > 0 and g["crack_px"] == kept.sum() and a["crack_px"] == region.sum()
            tops.append((g["name"], _check_topology_keys(g, skel, int(kept.sum()))))
            _check_topology_keys(a, skel_all, int(region.sum()))
            rows = TC.topology_rows(lab, TC.topo_of(skel)[None], k)
            assert len(rows) == len(g["cracks"]) == len(c["cracks"]) >= 2
            for crack, plain, row in zip(g["cracks"], c["cracks"], rows.tolist()):
                assert set(crack) == set(plain) | CRACK_TOPOLOGY_KEYS and {q: crack[q] for q in plain} == plain
                assert crack["y"] * W + crack["x"] + 1 == row[1]
                assert {q: crack[q] for q in CRACK_TOPOLOGY_KEYS} == TC.crack_of(row[2:], crack["length_px"])
                assert crack["loops"] == TC.holes(skel & (lab[0] == row[1])) and type(crack["loops"]) is int
                assert type(crack["length_geodesic_px"]) is float and type(crack["links"]) is tuple
            assert sum(crack["endpoints"] for crack in g["cracks"]) == g["endpoints"]
            assert sum(crack["junctions"] for crack in g["cracks"]) == g["junctions"] and sum(crack["loops"] for crack in g["cracks"]) == g["loops"]
            assert tuple(sum(crack["links"][i] for crack in g["cracks"]) for i in range(4)) == g["links"]
            # with the width too: both sets of keys, the same values
            for key in TOPOLOGY_KEYS:
                assert torch.equal(b[key], g[key]) if torch.is_tensor(g[key]) else b[key] == g[key], key
            assert [{q: crack[q] for q in CRACK_TOPOLOGY_KEYS} for crack in b["cracks"]] == [{q: crack[q] for q in CRACK_TOPOLOGY_KEYS} for crack in g["cracks"]]
            assert all("max_width_px" in crack and "widest" in crack for crack in b["cracks"])
            # nothing else changes with the option
            _same({q: g[q] for q in crack_keys - {"cracks"}}, {q: c[q] for q in crack_keys - {"cracks"}})
            _same({q: a[q] for q in measure_keys}, m)
            inst.append((g["name"], [{q: crack[q] for q in CRACK_TOPOLOGY_KEYS} for crack in g["cracks"]]))
        assert sorted(os.listdir(save)) == ["crack_instance_topology.csv", "crack_instances.csv", "crack_stats.csv", "crack_topology.csv", "images",
                                            "kernels", "kernels_origin", "masks", "skeletons"]
        assert sorted(os.listdir(save_w)) == ["crack_stats.csv", "crack_topology.csv", "images", "kernels", "kernels_origin", "masks", "skeletons"]
        assert SC.read_csv(str(save / "crack_topology.csv"))[0] == I.TOPOLOGY_CSV_COLUMNS
        assert I.read_crack_topology(str(save / "crack_topology.csv")) == tops
        assert SC.read_csv(str(save / "crack_instance_topology.csv"))[0] == I.INSTANCE_TOPOLOGY_COLUMNS
        assert I.read_crack_instance_topology(str(save / "crack_instance_topology.csv")) == inst
        assert [n for n, _ in I.read_crack_instances(str(save / "crack_instances.csv"))] == names      # the same numbering
    # topology=False is the call without the argument: the same keys, values and files
    for kwargs in (dict(), dict(measure_threshold=t), dict(measure_threshold=t, min_crack_px=k), dict(measure_threshold=t, min_crack_px=k, width_radius=5)):
        tag = "_".join(sorted(kwargs)) or "plain"
        off = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_off"), topology=False, **kwargs))
        none = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_none"), **kwargs))
        assert len(off) == len(none) == 2
        for x, y in zip(off, none):
            cx, cy = x.pop("cracks", None), y.pop("cracks", None)
            hx, hy = x.pop("width_hist", None), y.pop("width_hist", None)
            _same(x, y)
            assert cx == cy and (hx is None) == (hy is None) and (hx is None or np.array_equal(hx, hy))
            assert not (set(x) & TOPOLOGY_KEYS)
        fa, fb = _files(tmp_path / f"{tag}_off"), _files(tmp_path / f"{tag}_none")
        assert fa == fb and not any("topology" in n for n in fa)
    # an all-zero map
    zero = lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs))
    for kwargs in (dict(), dict(min_crack_px=k)):
        g = next(predict_dataset(zero, ld, measure_threshold=t, topology=True, **kwargs))
        assert (g["endpoints"], g["junctions"], g["junction_px"], g["isolated_px"], g["loops"], g["links"], g["length_geodesic_px"], g["orientation"],
                g["mean_width_geodesic_px"]) == (0, 0, 0, 0, 0, (0, 0, 0, 0), 0.0, (0.0, 0.0, 0.0, 0.0), 0.0)
        assert int(g["topology_map"].sum()) == 0
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(topology=True), dict(min_crack_px=k, topology=True), dict(measure_threshold=t, topology=1), dict(measure_threshold=t, topology=None),
                   dict(measure_threshold=t, topology="True"), dict(measure_threshold=t, min_crack_px=k, topology=0)):
        with pytest.raises(ValueError):
            next(predict_dataset(model, ld, **kwargs))
