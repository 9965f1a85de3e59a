"""csrc/branches.hip and its drivers on the device: every result is an integer and is asked for exactly, against the NumPy restatement of
tests/branch_cases.py (whose own properties tests/test_branches_cpu.py holds).

Through the C ABI the topo bytes sit inside an allocation filled with 0xF3 -- a path pixel that owns all four links, so a read outside a
plane would add a branch pixel or a link --, the labels and the width map between label-like values, and every output inside a
sentinel-filled allocation whose margins are checked; the slots of ``bacc`` that belong to no root must still hold the sentinel."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import branch_cases as BC
import components_cases as CC
import skeleton_cases as SC
import topology_cases as TC

pytestmark = pytest.mark.gpu

PAD = 64
ISENT = 0x5A5A5A5A
LINKED = 0xF3                                                                        # class 3 with the E, S, SE and SW link
DEV = torch.device("cuda", 0)
COL = {k: j for j, k in enumerate(BC.COLUMNS)}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _inp(x, fill, dtype, pad):
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


def device_blabels(topo):
    """int32 [N, H, W] of csbsr_branch_label through the C ABI"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = topo.shape
    _, t = _inp(topo, LINKED, torch.uint8, 2 * (W + 2))                              # linked branch pixels before the first and behind the last plane
    (ww, work), (wb, bl) = _out(N * H * W), _out(N * H * W)
    L.call("csbsr_branch_label", _ptr(t), N, H, W, _ptr(work), _ptr(bl), _stream())
    torch.cuda.synchronize()
    _margins_intact(ww, wb)
    return bl.cpu().numpy().reshape(N, H, W)


def device_bacc(blabels, topo, jlabels=None, d2=None):
    """int32 [N, 12 or 14, H W] of csbsr_branch_sums through the C ABI, the sentinel where nothing was written"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = blabels.shape
    K = 12 if d2 is None else 14
    pad = 2 * (W + 2)
    _, bl = _inp(blabels, 1, torch.int32, pad)
    _, t = _inp(topo, LINKED, torch.uint8, pad)
    jl = None if jlabels is None else _inp(jlabels, 1, torch.int32, pad)[1]
    dd = None if d2 is None else _inp(d2, 7, torch.int32, pad)[1]
    wa, bacc = _out(N * K * H * W)
    L.call("csbsr_branch_sums", _ptr(bl), _ptr(t), None if jl is None else _ptr(jl), None if dd is None else _ptr(dd), N, H, W, _ptr(bacc), _stream())
    torch.cuda.synchronize()
    _margins_intact(wa)
    return bacc.cpu().numpy().reshape(N, K, H * W)


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", list(BC.cases()))
def test_labels_and_sums_equal_the_restatement(name):
    """the shapes of topology_cases.SHAPES (1 x 1 up to 130 x 260: 3 x 3 tiles), the seams and borders, diagonal strokes over a four-tile
    corner, a T with its junction on a seam, noise at four densities, the crack skeletons and their pruned forms, all ones, all zeros and a
    plane of ones between planes of zeros"""
    topo, want, jl = BC.expected(name)
    got = device_blabels(topo)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    d2 = BC.fake_d2(want)
    bacc = device_bacc(got, topo, jl, d2)
    assert np.array_equal(bacc, BC.bacc_of(topo, want, jl, d2, fill=ISENT)), np.argwhere(bacc != BC.bacc_of(topo, want, jl, d2, fill=ISENT))[:5]
    # every link falls into exactly one of inner, attach and cluster
    N, H, W = topo.shape
    roots = want.reshape(N, H * W) == np.arange(1, H * W + 1)
    for n in range(N):
        inner, attach, cluster = (len(p) for p in BC.partition(topo[n]))
        counts = TC.counts_of(topo[n])
        sums = bacc[n][:, roots[n]].astype(np.int64)
        assert sums[3:7].sum() == inner + attach and sums[2].sum() == attach and inner + attach + cluster == counts[5:9].sum()
        assert sums[0].sum() == counts[0] - counts[4] and sums[1].sum() == counts[2]


def test_the_crack_skeletons_have_their_branches_on_the_device():
    topo = BC.expected("cracks")[0]
    bl = device_blabels(topo)
    N, H, W = bl.shape
    roots = bl.reshape(N, H * W) == np.arange(1, H * W + 1)
    assert roots.sum(1).tolist() == [BC.BRANCH_COUNTS[s] for s in TC.CRACK_SEEDS]
    bacc = device_bacc(bl, topo)
    for n, seed in enumerate(TC.CRACK_SEEDS):
        inner, attach, cluster = BC.PARTITIONS[seed]
        sums = bacc[n][:, roots[n]].astype(np.int64)
        assert (sums[3:7].sum(), sums[2].sum()) == (inner + attach, attach) and TC.counts_of(topo[n])[5:9].sum() == inner + attach + cluster


@pytest.mark.parametrize("name", ["cracks", "noise_0.3", "corner_strokes", "seam_T"])
@pytest.mark.parametrize("with_jl", [False, True])
@pytest.mark.parametrize("with_d2", [False, True])
def test_each_sum_with_and_without_junction_labels_and_a_width_map(name, with_jl, with_d2):
    topo, bl, jl = BC.expected(name)
    d2 = BC.fake_d2(bl, seed=4) if with_d2 else None
    got = device_bacc(bl, topo, jl if with_jl else None, d2)
    assert got.shape[1] == (14 if with_d2 else 12)
    assert np.array_equal(got, BC.bacc_of(topo, bl, jl if with_jl else None, d2, fill=ISENT))


def test_the_T_on_device_has_three_labels():
    plane = BC.hand("T")
    bl = device_blabels(TC.topo_of(plane)[None])[0]
    assert len(set(bl[bl != 0].tolist())) == 3 and bl[2, 5] == 0 and ((bl != 0) == (plane != 0) & ~BC.is_junction(TC.topo_of(plane))).all()


def test_two_runs_are_bit_equal():
    for name in ("noise_0.6", "cracks", "corner_strokes", "noise_130x260"):
        topo, _, jl = BC.expected(name)
        a, b = device_blabels(topo), device_blabels(topo)
        assert np.array_equal(a, b)
        d2 = BC.fake_d2(a)
        assert np.array_equal(device_bacc(a, topo, jl, d2), device_bacc(b, topo, jl, d2))


def test_the_tile_getter_names_the_seams():
    from csbsr_amd import _lib as L
    L.load()
    th, tw = C.c_int32(0), C.c_int32(0)
    L.call("csbsr_branch_tile", C.byref(th), C.byref(tw))
    assert (th.value, tw.value) == (BC.TH, BC.TW)


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    L.load()
    topo = torch.full((64,), LINKED, dtype=torch.uint8, device=DEV)
    lab = torch.ones(64, dtype=torch.int32, device=DEV)
    work, bl, bacc = (torch.full((n,), ISENT, dtype=torch.int32, device=DEV) for n in (64, 64, 14 * 64))
    st = _stream()
    good = dict(N=1, H=8, W=8)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(H=-8), dict(W=-8), dict(H=8193), dict(W=8193), dict(N=65536)):
        d = {**good, **bad}
        dims = (d["N"], d["H"], d["W"])
        for call in (("csbsr_branch_label", _ptr(topo), *dims, _ptr(work), _ptr(bl), st),
                     ("csbsr_branch_sums", _ptr(lab), _ptr(topo), _ptr(lab), _ptr(lab), *dims, _ptr(bacc), st),
                     ("csbsr_branch_sums", _ptr(lab), _ptr(topo), None, None, *dims, _ptr(bacc), st)):
            with pytest.raises(L.CsbsrHipError):
                L.call(*call)
    for call in (("csbsr_branch_label", None, 1, 8, 8, _ptr(work), _ptr(bl), st),
                 ("csbsr_branch_label", _ptr(topo), 1, 8, 8, None, _ptr(bl), st),
                 ("csbsr_branch_label", _ptr(topo), 1, 8, 8, _ptr(work), None, st),
                 ("csbsr_branch_label", _ptr(topo), 1, 8, 8, _ptr(bl), _ptr(bl), st),                   # work is another array than blabels
                 ("csbsr_branch_sums", None, _ptr(topo), None, None, 1, 8, 8, _ptr(bacc), st),
                 ("csbsr_branch_sums", _ptr(lab), None, None, None, 1, 8, 8, _ptr(bacc), st),
                 ("csbsr_branch_sums", _ptr(lab), _ptr(topo), None, None, 1, 8, 8, None, st),
                 ("csbsr_branch_tile", None, None)):
        with pytest.raises(L.CsbsrHipError):
            L.call(*call)
    torch.cuda.synchronize()
    for t in (work, bl, bacc):                                                       # nothing ran: no output was written
        assert bool((t == ISENT).all())


# ------------------------------------------------------------------------------------------------ the Python surface
def test_label_branches_and_branch_table_surface():
    from csbsr_amd.utils import estimate_metrics as M
    for name in ("cracks", "corner_strokes", "noise_0.3", "ones_between_zeros", "zeros"):
        topo_np, bl_np, jl_np = BC.expected(name)
        N, H, W = topo_np.shape
        topo = torch.from_numpy(topo_np).to(DEV)
        bl = M.label_branches(topo)
        assert bl.is_cuda and bl.dtype == torch.int32 and tuple(bl.shape) == (N, H, W) and np.array_equal(bl.cpu().numpy(), bl_np)
        assert torch.equal(M.label_branches(torch.from_numpy(topo_np)), bl)          # a CPU tensor
        jl = M._junction_labels(topo)
        assert np.array_equal(jl.cpu().numpy(), jl_np)
        lab_np = np.stack([CC.canonical_labels(p != 0, 8) for p in BC.cases()[name]])
        lab = torch.from_numpy(lab_np).to(DEV)
        d2_np = BC.fake_d2(bl_np)
        d2 = torch.from_numpy(d2_np).to(DEV)
        for kwargs, want in ((dict(), BC.rows_of(topo_np, jlabels=None)),
                             (dict(jlabels=jl), BC.rows_of(topo_np)),
                             (dict(jlabels=jl, labels=lab), BC.rows_of(topo_np, labels=lab_np)),
                             (dict(jlabels=jl, d2=d2), BC.rows_of(topo_np, d2=d2_np)),
                             (dict(jlabels=jl, labels=lab, d2=d2), BC.rows_of(topo_np, labels=lab_np, d2=d2_np))):
            got = M.branch_table(bl, topo, **kwargs)
            assert got.is_cuda and got.dtype == torch.int32 and got.dim() == 2 and got.shape[1] == (19 if "d2" in kwargs else 17)
            assert np.array_equal(got.cpu().numpy(), want), sorted(kwargs)
        rows = M.branch_table(bl, topo, jl).cpu().numpy()
        assert M.branch_kinds(rows) == BC.kinds_of(rows)
    topo = torch.from_numpy(BC.expected("cracks")[0]).to(DEV)
    bl = M.label_branches(topo)
    for bad in (dict(jlabels=bl[:, :-1]), dict(labels=bl.to(torch.int64)), dict(d2=bl.to(torch.float32)), dict(jlabels=bl[0])):
        with pytest.raises(ValueError):
            M.branch_table(bl, topo, **bad)
    for bad in ((bl, topo[:, :-1]), (bl, topo.to(torch.int32)), (bl.to(torch.int64), topo), (bl.cpu(), topo), (bl[0], topo[0])):
        with pytest.raises(ValueError):
            M.branch_table(*bad)
    for bad in (topo.to(torch.int32), topo[0], topo.cpu().numpy()):
        with pytest.raises(ValueError):
            M.label_branches(bad)


# ------------------------------------------------------------------------------------------------ the driver
BRANCH_KEYS = {"n_branches", "branch_kinds", "longest_branch_px", "branch_map", "branches"}
BRANCH_DICT_KEYS = {"y", "x", "kind", "px", "ends", "attach", "nodes", "links", "length_geodesic_px", "orientation", "bbox"}


def _same(a, b):
    """two yielded dicts hold the same keys and the same values"""
    assert set(a) == set(b)
    for key in a:
        if torch.is_tensor(a[key]):
            assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key
        elif isinstance(a[key], np.ndarray):
            assert np.array_equal(a[key], b[key]), key
        else:
            assert type(a[key]) is type(b[key]) and a[key] == b[key], key


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            with open(os.path.join(d, n), "rb") as fh:
                out[os.path.relpath(os.path.join(d, n), root)] = fh.read()
    return out


def _check_branch_keys(g, skel, labels=None, d2=None):
    """the new keys of one yielded dict against the skeleton bool [H, W] of the NumPy chain; returns the branches list"""
    from csbsr_amd.utils import estimate_metrics as M
    H, W = skel.shape
    topo = TC.topo_of(skel)
    rows = BC.rows_of(topo[None], labels=None if labels is None else labels[None], d2=None if d2 is None else d2[None])
    of_label = None if labels is None else {c["y"] * W + c["x"] + 1: j for j, c in enumerate(g["cracks"])}
    want = BC.branch_dicts(rows, W, of_label)
    assert g["branches"] == want and g["n_branches"] == len(want) and type(g["n_branches"]) is int
    kinds = [b["kind"] for b in want]
    assert g["branch_kinds"] == {k: kinds.count(k) for k in BC.KINDS} and list(g["branch_kinds"]) == list(BC.KINDS)
    lengths = [b["length_geodesic_px"] for b in want if b["kind"] != "isolated"]
    assert g["longest_branch_px"] == (max(lengths) if lengths else 0.0) and type(g["longest_branch_px"]) is float
    assert g["branch_map"].is_cuda and g["branch_map"].dtype == torch.int32 and np.array_equal(g["branch_map"].cpu().numpy(), BC.blabels_of(topo))
    for b in g["branches"]:
        assert set(b) == BRANCH_DICT_KEYS | ({"crack"} if labels is not None else set()) | ({"max_width_px", "min_width_px"} if d2 is not None else set())
        assert type(b["px"]) is int and type(b["length_geodesic_px"]) is float and type(b["nodes"]) is tuple and type(b["bbox"]) is tuple
    assert sum(b["ends"] for b in want) == g["endpoints"] and kinds.count("isolated") == g["isolated_px"]
    assert sum(b["px"] for b in want) == g["skeleton_px"] - g["junction_px"]
    if labels is not None:
        for j, c in enumerate(g["cracks"]):
            assert c["n_branches"] == sum(1 for b in want if b["crack"] == j) and type(c["n_branches"]) is int
        assert sum(c["n_branches"] for c in g["cracks"]) == g["n_branches"]
    return want


def test_predict_dataset_with_branches(tmp_path):
    """test_predict_dataset_with_min_crack_px's two images (stitched maps of 64 x 96 and 84 x 68), with the branch table of the skeleton the
    call reports: whole, kept with min_crack_px, pruned with prune_spur_px, and with the width columns of width_radius"""
    import eval_io_cases as EC
    import predict_cases as PC
    import prune_cases as PR
    import width_cases as WC
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd import inference as I
    predict_dataset = I.predict_dataset
    images = PC.make_images(PC.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t, k, r, Lp = 0.4, 5, 64, 6
    base = dict(measure_threshold=t, topology=True)
    total = 0
    for batch_patches in (16, 4):                                                   # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        want = PC.host_chain(ld, images, EC.stub_model, torch.from_numpy, EC.thresholds32()[EC.SAVE_IDX])
        chain = []                                                                   # the NumPy chain of every image, once
        for w in want:
            region = SC.binarise(w["map_f32"], t)
            lab = CC.canonical_labels(region, 8)[None]
            skel_all = SC.skeleton(region)
            chain.append(dict(region=region, lab=lab[0], kept=CC.keep(lab, k)[0].astype(bool), skel=skel_all, pruned=PR.prune(skel_all, Lp)[0].astype(bool),
                              d2=WC.d2_of(region, r)))
        options = {"whole": dict(), "kept": dict(min_crack_px=k), "width": dict(width_radius=r), "pruned": dict(prune_spur_px=Lp),
                   "all": dict(min_crack_px=k, width_radius=r, prune_spur_px=Lp)}
        for tag, opt in options.items():
            on_dir, off_dir = tmp_path / f"{batch_patches}_{tag}_on", tmp_path / f"{batch_patches}_{tag}_off"
            on = list(predict_dataset(EC.stub_model, ld, save_dir=str(on_dir), branches=True, **base, **opt))
            off = list(predict_dataset(EC.stub_model, ld, save_dir=str(off_dir), **base, **opt))
            csv_rows = []
            for g, o, ch in zip(on, off, chain):
                assert set(g) == set(o) | BRANCH_KEYS
                skel = ch["pruned"] if "prune_spur_px" in opt else ch["skel"]
                labels = None
                if "min_crack_px" in opt:
                    skel, labels = skel & ch["kept"], (ch["lab"] * ch["kept"]).astype(np.int32)
                d2 = np.where(skel, ch["d2"], 0).astype(np.int32) if "width_radius" in opt else None
                assert skel.sum() > 0 and g["skeleton_px"] == skel.sum()
                blist = _check_branch_keys(g, skel, labels, d2)
                total += len(blist)
                csv_rows.append((g["name"], blist))
                # every key of the call without the option is bit-equal
                gc = [{q: v for q, v in c.items() if q != "n_branches"} for c in g.get("cracks", [])]
                _same({q: v for q, v in g.items() if q not in BRANCH_KEYS | {"cracks"}}, {q: v for q, v in o.items() if q != "cracks"})
                assert gc == o.get("cracks", []) and all("n_branches" not in c for c in o.get("cracks", []))
            fa, fb = _files(on_dir), _files(off_dir)
            assert set(fa) == set(fb) | {"crack_branches.csv"} and all(fa[n] == fb[n] for n in fb)      # and so is every file
            assert I.read_crack_branches(str(on_dir / "crack_branches.csv")) == csv_rows
            header = SC.read_csv(str(on_dir / "crack_branches.csv"))[0]
            assert header == I.BRANCH_CSV_COLUMNS + (["crack"] if "min_crack_px" in opt else []) + (["max_width_px", "min_width_px"] if "width_radius" in opt else [])
    assert total > 20, "the maps have branches"
    # branches=False is the call without the argument: the same keys, values and files
    for kwargs in (dict(), dict(measure_threshold=t), dict(measure_threshold=t, topology=True), dict(measure_threshold=t, min_crack_px=k, width_radius=5, topology=True)):
        tag = "_".join(sorted(kwargs)) or "plain"
        off = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_off"), branches=False, **kwargs))
        none = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_none"), **kwargs))
        assert len(off) == len(none) == 2
        for x, y in zip(off, none):
            _same(x, y)
            assert not (set(x) & BRANCH_KEYS)
        fa, fb = _files(tmp_path / f"{tag}_off"), _files(tmp_path / f"{tag}_none")
        assert fa == fb and not any("branches" in n for n in fa)
    # an all-zero map has no branch
    zero = lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs))
    for kwargs in (dict(), dict(min_crack_px=k), dict(width_radius=5, prune_spur_px=3)):
        g = next(predict_dataset(zero, ld, branches=True, **base, **kwargs))
        assert (g["n_branches"], g["branch_kinds"], g["longest_branch_px"], g["branches"]) == (0, {q: 0 for q in BC.KINDS}, 0.0, [])
        assert int(g["branch_map"].sum()) == 0
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(branches=True), dict(measure_threshold=t, branches=True), dict(measure_threshold=t, topology=True, branches=1),
                   dict(measure_threshold=t, topology=True, branches=None), dict(measure_threshold=t, topology=True, branches="True")):
        with pytest.raises(ValueError):
            next(predict_dataset(model, ld, **kwargs))
