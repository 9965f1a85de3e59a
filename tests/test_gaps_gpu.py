"""csrc/gaps.hip and its drivers on the device: every output is an integer and is asked for exactly, at every pixel, for both targets and
every gap, against the NumPy restatement of tests/gap_cases.py (whose own properties tests/test_gaps_cpu.py holds).

Through the C ABI the planes sit between bytes that read as set pixels and labels that read as other cracks, every output inside a
sentinel-filled allocation whose margins are checked: nothing outside a plane may be read as a candidate, nothing outside an output
written, and nothing may depend on what an output held."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gap_cases as GC

pytestmark = pytest.mark.gpu

PAD = 1 << 15                                                                        # more than 64 rows of the widest plane
ISENT = 0x5A5A5A5A
BSENT = 0x5A
DEV = torch.device("cuda", 0)


def _ptr(t):
    return C.c_void_p(t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _inp(x, fill, dtype):
    x = torch.from_numpy(np.array(x)).to(dtype).reshape(-1)                          # a copy: the cases are read-only
    buf = torch.full((x.numel() + 2 * PAD,), fill, dtype=dtype, device=DEV)
    buf[PAD:PAD + x.numel()] = x.to(DEV)
    return buf[PAD:PAD + x.numel()]


def _out(n, dtype=torch.int32):
    buf = torch.full((n + 2 * PAD,), BSENT if dtype == torch.uint8 else ISENT, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _margins_intact(*wholes):
    for w in wholes:
        sent = BSENT if w.dtype == torch.uint8 else ISENT
        assert bool((w[:PAD] == sent).all()) and bool((w[-PAD:] == sent).all()), "a write outside an output"


def device_all(topo, labels, G, to):
    """(gap_q, gap_d2, group_labels, bridge_map) through the C ABI: the planes between end pixels (0xFA: class 2) of label 77"""
    from csbsr_amd import _lib as L
    N, H, W = topo.shape
    t, lab = _inp(topo, 0xFA, torch.uint8), _inp(labels, 77, torch.int32)
    (wq, gq), (wd, gd), (wp, parent), (wg, groups) = (_out(N * H * W) for _ in range(4))
    wb, bridges = _out(N * H * W, torch.uint8)
    L.call("csbsr_endpoint_gaps", _ptr(t), _ptr(lab), N, H, W, G, int(to == "end"), _ptr(gq), _ptr(gd), _stream())
    L.call("csbsr_gap_groups", _ptr(lab), _ptr(gq), N, H, W, _ptr(parent), _ptr(groups), _stream())
    L.call("csbsr_gap_draw", _ptr(gq), N, H, W, _ptr(bridges), _stream())
    torch.cuda.synchronize()
    _margins_intact(wq, wd, wp, wg, wb)
    return tuple(v.cpu().numpy().reshape(N, H, W) for v in (gq, gd, groups, bridges))


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", list(GC.cases()))
def test_every_output_equals_the_restatement(name):
    """hand cases, ends across every seam of the 64 x 128 tiles and in the last word's remainder, a pair exactly 64 and one 65 apart across
    a whole tile, the broken cracks and the noise planes; outputs pre-filled with garbage are fully overwritten"""
    from csbsr_amd.utils import estimate_metrics as M
    topo, labels = GC.cases()[name]
    topo_d, labels_d = torch.from_numpy(np.array(topo)).to(DEV), torch.from_numpy(np.array(labels)).to(DEV)
    for G in GC.gaps_for(name):
        for to in GC.TOS:
            gq, gd, groups, bridges = device_all(topo, labels, G, to)
            wq, wd, wtable, wgroups, wbridges = GC.expected(name, G, to)
            table = M.gap_table(topo_d, labels_d, torch.from_numpy(gq).to(DEV), torch.from_numpy(gd).to(DEV))
            assert table.is_cuda and table.dtype == torch.int32 and np.array_equal(table.cpu().numpy(), wtable), (G, to)
            assert gq.dtype == np.int32 and np.array_equal(gq, wq), (G, to, np.argwhere(gq != wq)[:4])
            assert gd.dtype == np.int32 and np.array_equal(gd, wd), (G, to, np.argwhere(gd != wd)[:4])
            assert groups.dtype == np.int32 and np.array_equal(groups, wgroups), (G, to, np.argwhere(groups != wgroups)[:4])
            assert bridges.dtype == np.uint8 and np.array_equal(bridges, wbridges), (G, to, np.argwhere(bridges != wbridges)[:4])


def test_the_pinned_counts_and_two_runs_are_bit_equal():
    for mask in GC.CRACK_MASKS:
        topo, labels = GC.crack_case(mask)
        runs = [device_all(topo, labels, G, "any") for G in GC.CRACK_GAPS]
        assert tuple(int((r[0] >= 0).sum()) for r in runs) == GC.CRACK_COUNTS[mask]
        again = device_all(topo, labels, GC.CRACK_GAPS[-1], "any")
        assert all(np.array_equal(a, b) for a, b in zip(runs[-1], again))
    for name in ("noise_0.3", "noise_0.6", "tile_seams"):
        topo, labels = GC.cases()[name]
        a, b = device_all(topo, labels, 64, "any"), device_all(topo, labels, 64, "any")
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    from csbsr_amd.utils import estimate_metrics as M
    lib = L.load()
    assert int(lib.csbsr_gap_max_radius()) == 64 == M.GAP_MAX_RADIUS
    topo = torch.zeros(64, dtype=torch.uint8, device=DEV)
    labels = torch.zeros(64, dtype=torch.int32, device=DEV)
    a, b, c = (torch.full((64,), ISENT, dtype=torch.int32, device=DEV) for _ in range(3))
    bm = torch.full((64,), BSENT, dtype=torch.uint8, device=DEV)
    st = _stream()
    search = lambda **k: ("csbsr_endpoint_gaps", k.get("topo", _ptr(topo)), k.get("labels", _ptr(labels)), k.get("N", 1), k.get("H", 8), k.get("W", 8),
                          k.get("G", 4), k.get("to_end", 0), k.get("q", _ptr(a)), k.get("d2", _ptr(b)), st)
    group = lambda **k: ("csbsr_gap_groups", k.get("labels", _ptr(labels)), k.get("q", _ptr(a)), k.get("N", 1), k.get("H", 8), k.get("W", 8),
                         k.get("parent", _ptr(b)), k.get("groups", _ptr(c)), st)
    draw = lambda **k: ("csbsr_gap_draw", k.get("q", _ptr(a)), k.get("N", 1), k.get("H", 8), k.get("W", 8), k.get("map", _ptr(bm)), st)
    calls = [search(**{k: None}) for k in ("topo", "labels", "q", "d2")] + [group(**{k: None}) for k in ("labels", "q", "parent", "groups")]
    calls += [draw(q=None), draw(map=None)]
    calls += [search(G=g) for g in (1, 0, -1, 65, 128)] + [search(to_end=2), search(to_end=-1)]
    for f in (search, group, draw):
        calls += [f(H=0), f(W=0), f(H=8193), f(W=8193), f(N=0), f(N=65536), f(H=-1)]
    calls += [search(q=_ptr(b)), search(q=_ptr(labels)), search(d2=_ptr(labels)), group(parent=_ptr(c)), group(parent=_ptr(labels)), group(parent=_ptr(a))]
    for call in calls:
        with pytest.raises(L.CsbsrHipError):
            L.call(*call)
    torch.cuda.synchronize()
    for t, sent in ((a, ISENT), (b, ISENT), (c, ISENT), (bm, BSENT)):                # nothing ran: no output was written
        assert bool((t == sent).all())


# ------------------------------------------------------------------------------------------------ the Python surface
def test_the_python_surface():
    from csbsr_amd.utils import estimate_metrics as M
    for name in ("tile_seams", "two_planes", "cracks_6_131x135", "noise_0.3", "u_shape"):
        topo_np, labels_np = GC.cases()[name]
        topo, labels = torch.from_numpy(np.array(topo_np)).to(DEV), torch.from_numpy(np.array(labels_np)).to(DEV)
        for G, to in ((2, "any"), (5, "end"), (16, "any"), (64, "end")):
            wq, wd, wtable, wgroups, wbridges = GC.expected(name, G, to)
            gq, gd = M.endpoint_gaps(topo, labels, G, to)
            assert all(t.is_cuda and t.dtype == torch.int32 and tuple(t.shape) == topo_np.shape for t in (gq, gd))
            assert np.array_equal(gq.cpu().numpy(), wq) and np.array_equal(gd.cpu().numpy(), wd)
            table = M.gap_table(topo, labels, gq, gd)
            assert table.is_cuda and table.dtype == torch.int32 and tuple(table.shape) == wtable.shape and np.array_equal(table.cpu().numpy(), wtable)
            groups, bridges = M.gap_groups(labels, gq), M.draw_bridges(gq)
            assert groups.is_cuda and groups.dtype == torch.int32 and np.array_equal(groups.cpu().numpy(), wgroups)
            assert bridges.is_cuda and bridges.dtype == torch.uint8 and np.array_equal(bridges.cpu().numpy(), wbridges)
            assert torch.equal(M.gap_groups(groups, gq), groups)                     # grouping twice changes nothing
    assert np.array_equal(M.endpoint_gaps(topo, labels, np.int64(5))[0].cpu().numpy(), GC.expected("u_shape", 5, "any")[0])
    # the labels of the device's own labelling and topology
    import components_cases as CC
    import skeleton_cases as SC
    img = CC.broken_cracks(*GC.CRACK_MASKS[2])
    x = torch.from_numpy(img.astype(np.float32)).to(DEV)[None]
    sk = M.skeletonize(x, 0.5)
    gq, gd = M.endpoint_gaps(M.skeleton_topology(sk)[0], M.label_components(x, 0.5), 8)
    assert np.array_equal(gq.cpu().numpy(), GC.expected("cracks_4_70x133", 8, "any")[0]) and np.array_equal(sk.cpu().numpy()[0], SC.skeleton(img))
    for bad in ((topo, labels, 1), (topo, labels, 65), (topo, labels, 4.0), (topo, labels, True), (topo, labels, 4, "side"), (topo, labels.long(), 4),
                (topo.to(torch.int32), labels, 4), (topo[0], labels, 4), (topo, labels[:, :-1], 4), (topo, labels.cpu(), 4)):
        with pytest.raises(ValueError):
            M.endpoint_gaps(*bad)
    for call in (lambda: M.gap_table(topo, labels, gq, gd), lambda: M.gap_groups(labels, gq), lambda: M.gap_groups(labels, gq.long()),
                 lambda: M.draw_bridges(gq.cpu()), lambda: M.draw_bridges(gq[0]), lambda: M.draw_bridges(gq.to(torch.uint8))):
        with pytest.raises(ValueError):                                              # gq belongs to another shape
            call()


# ------------------------------------------------------------------------------------------------ the driver
GAP_KEYS = {"n_gaps", "n_mutual_gaps", "gap_length_px", "max_gap_px", "bridge_px", "n_cracks_bridged", "gaps", "bridge_map", "bridged_labels"}
CRACK_GAP_KEYS = {"group", "gaps"}


def _same_value(a, b, key):
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and torch.equal(a, b), key
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), key
    elif isinstance(a, list) and a and isinstance(a[0], dict):
        assert len(a) == len(b), key
        for x, y in zip(a, b):
            _same(x, y)
    else:
        assert type(a) is type(b) and a == b, key


def _same(a, b):
    """two dicts hold the same keys and the same values"""
    assert set(a) == set(b)
    for key in a:
        _same_value(a[key], b[key], key)


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as fh:
                out[os.path.relpath(os.path.join(d, n), root)] = fh.read()
    return out


def _check_gap_keys(g, t, G, to, kept):
    """the new keys of one yielded dict against the restatement applied to the yielded topology_map and the labels the call names its
    cracks with; returns the number of gaps"""
    import components_cases as CC
    import skeleton_cases as SC
    topo = g["topology_map"].cpu().numpy()
    H, W = topo.shape
    region = CC.canonical_labels(SC.binarise(g["map_f32"].cpu().numpy(), t))
    labels = g["labels"].cpu().numpy() if kept else region
    assert not kept or ((labels == region) | (labels == 0)).all()
    sk = (topo & 7) != 0
    gq, gd = GC.gaps_brute(topo[None], labels[None], G, to)
    rows = GC.gap_table(topo[None], labels[None], gq, gd)
    groups, bridges = GC.groups_of(labels[None], gq)[0], GC.bridges_of(gq)[0]
    assert g["bridge_map"].is_cuda and g["bridge_map"].dtype == torch.uint8 and np.array_equal(g["bridge_map"].cpu().numpy(), bridges)
    assert g["bridged_labels"].is_cuda and g["bridged_labels"].dtype == torch.int32 and np.array_equal(g["bridged_labels"].cpu().numpy(), groups)
    of_label = {c["y"] * W + c["x"] + 1: k for k, c in enumerate(g["cracks"])} if kept else None
    assert g["gaps"] == GC.gap_dicts(rows, W, of_label)
    assert all(type(d["gap_px"]) is float and type(d["mutual"]) is bool and type(d["d2"]) is int and type(d["to"]) is tuple for d in g["gaps"])
    n_cracks = g["n_cracks"] if kept else len(np.unique(labels[sk]))
    want = GC.summary_of(rows, n_cracks)
    assert (g["n_gaps"], g["n_mutual_gaps"], g["max_gap_px"], g["n_cracks_bridged"]) == (want["n_gaps"], want["n_mutual"], want["max_gap_px"],
                                                                                           want["n_cracks_bridged"])
    assert all(type(g[k]) is int for k in ("n_gaps", "n_mutual_gaps", "bridge_px", "n_cracks_bridged")) and type(g["gap_length_px"]) is float
    assert abs(g["gap_length_px"] - want["gap_length_px"]) <= 2 * len(rows) * 2.0 ** -53 * want["gap_length_px"]       # two orders of an fp64 sum
    assert g["bridge_px"] == int(((bridges != 0) & ~sk).sum())
    assert g["n_cracks_bridged"] == len(np.unique(groups[labels != 0] if kept else groups[sk])) <= n_cracks
    if kept:                                                                         # crack / to_crack / group name the dicts of cracks
        for d in g["gaps"]:
            for idx, (y, x) in ((d["crack"], (d["y"], d["x"])), (d["to_crack"], d["to"])):
                c = g["cracks"][idx]
                assert labels[y, x] == c["y"] * W + c["x"] + 1
        for k, c in enumerate(g["cracks"]):
            first = g["cracks"][c["group"]]
            assert groups[c["y"], c["x"]] == first["y"] * W + first["x"] + 1 and c["group"] <= k and first["group"] == c["group"]
            assert c["gaps"] == sum(d["crack"] == k for d in g["gaps"])
    return len(rows)


def test_predict_dataset_with_bridge_gap_px(tmp_path):
    """test_predict_dataset_with_polylines' two images (stitched maps of 64 x 96 and 84 x 68) with the gaps of the skeleton the call
    reports: whole, kept with min_crack_px, pruned with prune_spur_px, next to the other options"""
    from PIL import Image
    import eval_io_cases as EC
    import predict_cases as PC2
    import skeleton_cases as SC
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd import inference as I
    predict_dataset = I.predict_dataset
    images = PC2.make_images(PC2.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t, k, Lp = 0.4, 5, 6
    base = dict(measure_threshold=t, topology=True)
    total = {}
    for batch_patches in (16, 4):                                                    # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        options = {"whole": (4, "any", dict()), "kept": (8, "any", dict(min_crack_px=k)), "ends": (16, "end", dict(min_crack_px=k)),
                   "pruned": (5, "any", dict(prune_spur_px=Lp)),
                   "all": (64, "any", dict(min_crack_px=k, width_radius=16, prune_spur_px=Lp, branches=True, polylines=True, simplify_px=1.0))}
        for tag, (G, to, opt) in options.items():
            on_dir, off_dir = tmp_path / f"{batch_patches}_{tag}_on", tmp_path / f"{batch_patches}_{tag}_off"
            on = list(predict_dataset(EC.stub_model, ld, save_dir=str(on_dir), bridge_gap_px=G, bridge_to=to, **base, **opt))
            off = list(predict_dataset(EC.stub_model, ld, save_dir=str(off_dir), **base, **opt))
            kept = "min_crack_px" in opt
            for g, o in zip(on, off):
                assert set(g) == set(o) | GAP_KEYS
                total[tag] = total.get(tag, 0) + _check_gap_keys(g, t, G, to, kept)
                # every key of the call without the option is bit-equal
                if kept:
                    assert all(set(c) == set(d) | CRACK_GAP_KEYS for c, d in zip(g["cracks"], o["cracks"]))
                    _same_value([{q: v for q, v in c.items() if q not in CRACK_GAP_KEYS} for c in g["cracks"]], o["cracks"], "cracks")
                _same({q: v for q, v in g.items() if q not in GAP_KEYS | {"cracks"}}, {q: v for q, v in o.items() if q != "cracks"})
            fa, fb = _files(on_dir), _files(off_dir)
            assert set(fa) == set(fb) | {"crack_gaps.csv"} | {os.path.join("skeletons_bridged", n) for n in names}
            assert all(fa[n] == fb[n] for n in fb)                                   # and so is every file
            back = dict(I.read_crack_gaps(str(on_dir / "crack_gaps.csv")))
            for g in on:
                assert back.get(g["name"], []) == g["gaps"]
                png = np.asarray(Image.open(str(on_dir / "skeletons_bridged" / g["name"])))
                want = ((((g["topology_map"] & 7) != 0) | (g["bridge_map"] != 0)).to(torch.uint8) * 255).cpu().numpy()
                assert png.dtype == np.uint8 and np.array_equal(png, want)
            assert SC.read_csv(str(on_dir / "crack_gaps.csv"))[0] == I.GAP_CSV_COLUMNS + (I.GAP_CSV_OPTIONAL if kept else [])
    print("gaps per option set:", total)
    assert all(v > 0 for v in total.values()), "the maps have gaps under every option set"
    # with prune_spur_px the gaps are those of the pruned skeleton: its topology map is the pruned one's, and it is what was searched
    pruned = list(predict_dataset(EC.stub_model, ld, bridge_gap_px=5, prune_spur_px=Lp, **base))
    plain = list(predict_dataset(EC.stub_model, ld, bridge_gap_px=5, **base))
    assert sum(g["spur_px"] for g in pruned) > 0
    for g, o in zip(pruned, plain):
        sk, sk_all = (g["topology_map"] & 7) != 0, (o["topology_map"] & 7) != 0
        assert bool((sk <= sk_all).all()) and all(bool(sk[d["y"], d["x"]]) and bool(sk[d["to"]]) for d in g["gaps"])
    # bridge_gap_px=None is the call without the argument: the same keys, values and files
    for kwargs in (dict(), dict(measure_threshold=t), dict(**base), dict(min_crack_px=k, width_radius=5, branches=True, **base)):
        tag = "_".join(sorted(kwargs)) or "plain"
        none = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_none"), bridge_gap_px=None, bridge_to="any", **kwargs))
        off = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_off"), **kwargs))
        assert len(off) == len(none) == 2
        for x, y in zip(none, off):
            assert not (set(x) & GAP_KEYS) and not any(set(c) & CRACK_GAP_KEYS for c in x.get("cracks", []))
            _same(x, y)
        fa, fb = _files(tmp_path / f"{tag}_none"), _files(tmp_path / f"{tag}_off")
        assert fa == fb and not any("gaps" in n or "bridged" in n for n in fa)
    want_keys = {"name", "sr_u8", "map_u8", "map_f32", "kernels"}                   # the keys of the call before this option existed
    assert set(next(predict_dataset(EC.stub_model, ld))) == want_keys
    assert set(next(predict_dataset(EC.stub_model, ld, **base))) == want_keys | {
        "crack_px", "skeleton_px", "mean_width_px", "endpoints", "junctions", "junction_px", "isolated_px", "loops", "links", "length_geodesic_px",
        "orientation", "mean_width_geodesic_px", "topology_map"}
    # an all-zero map has no gap
    zero = lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs))
    for kwargs in (dict(), dict(min_crack_px=k), dict(prune_spur_px=3)):
        g = next(predict_dataset(zero, ld, bridge_gap_px=8, **base, **kwargs))
        assert (g["n_gaps"], g["n_mutual_gaps"], g["gap_length_px"], g["max_gap_px"], g["bridge_px"], g["n_cracks_bridged"], g["gaps"]) == (0, 0, 0.0, 0.0, 0, 0, [])
        assert not bool(g["bridge_map"].any()) and not bool(g["bridged_labels"].any())
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(bridge_gap_px=4), dict(bridge_gap_px=4, measure_threshold=t), dict(bridge_gap_px=1, **base), dict(bridge_gap_px=65, **base),
                   dict(bridge_gap_px=True, **base), dict(bridge_gap_px=4.0, **base), dict(bridge_gap_px=4, bridge_to="side", **base),
                   dict(bridge_to="end", **base), dict(bridge_to="end")):
        with pytest.raises(ValueError):
            next(predict_dataset(model, ld, **kwargs))
