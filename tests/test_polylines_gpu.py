"""csrc/polylines.hip and its drivers on the device: every result is an integer and is asked for exactly, at every pixel, against the NumPy
restatement of tests/polyline_cases.py (whose own properties tests/test_polylines_cpu.py holds).

Through the C ABI the topo bytes sit inside an allocation filled with 0xF3 -- a path pixel that owns all four links, so a read outside a
plane would add a branch pixel or a link --, the labels between label-like values, and every output inside a sentinel-filled allocation
whose margins are checked."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import branch_cases as BC
import components_cases as CC
import polyline_cases as PC
import skeleton_cases as SC
import topology_cases as TC

pytestmark = pytest.mark.gpu

PAD = 64
ISENT = 0x5A5A5A5A
LINKED = 0xF3                                                                        # class 3 with the E, S, SE and SW link
DEV = torch.device("cuda", 0)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _inp(x, fill, dtype, pad):
    x = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape(-1)
    buf = torch.full((x.numel() + 2 * pad,), fill, dtype=dtype, device=DEV)
    buf[pad:pad + x.numel()] = x.to(DEV)
    return buf[pad:pad + x.numel()]


def _out(n):
    buf = torch.full((n + 2 * PAD,), ISENT, dtype=torch.int32, device=DEV)
    return buf, buf[PAD:PAD + n]


def _margins_intact(*wholes):
    for w in wholes:
        assert bool((w[:PAD] == ISENT).all()) and bool((w[-PAD:] == ISENT).all()), "a write outside an output"


def device_order(topo, blabels):
    """(rank, diag int32 [N, H, W], P, R) of csbsr_branch_count and csbsr_branch_order through the C ABI"""
    from csbsr_amd import _lib as L
    lib = L.load()
    N, H, W = topo.shape
    t = _inp(topo, LINKED, torch.uint8, 2 * (W + 2))                                 # linked branch pixels before the first and behind the last plane
    bl = _inp(blabels, 1, torch.int32, 2 * (W + 2))
    count = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    L.call("csbsr_branch_count", _ptr(t), N, H, W, _ptr(count[1:]), _stream())
    assert count[0] == -7 and count[2] == -7
    P = int(count[1])
    assert P == int(BC.is_branch(topo).sum())
    need = int(lib.csbsr_branch_order_work_bytes(P))
    assert need >= 256 + 100 * P and need % 4 == 0
    ww, work = _out(need // 4)
    (wr, rank), (wd, diag) = _out(N * H * W), _out(N * H * W)
    L.call("csbsr_branch_order", _ptr(t), _ptr(bl), N, H, W, P, _ptr(work), _ptr(rank), _ptr(diag), _stream())
    torch.cuda.synchronize()
    _margins_intact(ww, wr, wd)
    return rank.cpu().numpy().reshape(N, H, W), diag.cpu().numpy().reshape(N, H, W), P, int(lib.csbsr_branch_order_rounds(P))


def device_points(blabels, rank, diag, offsets, rows, d2=None):
    """int32 [rows, 4] of csbsr_branch_scatter through the C ABI, the sentinel where nothing was written; ``offsets`` int32 [N, H W]"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = blabels.shape
    pad = 2 * (W + 2)
    bl, rk, dg, off = (_inp(a, f, torch.int32, pad) for a, f in ((blabels, 1, ), (rank, 0), (diag, 0), (offsets, 3)))
    dd = None if d2 is None else _inp(d2, 7, torch.int32, pad)
    wp, points = _out(4 * max(rows, 1))
    L.call("csbsr_branch_scatter", _ptr(bl), _ptr(rk), _ptr(dg), None if dd is None else _ptr(dd), _ptr(off), N, H, W, rows, _ptr(points), _stream())
    torch.cuda.synchronize()
    _margins_intact(wp)
    return points.cpu().numpy().reshape(-1, 4)[:rows]


def _offset_planes(blabels, chain, offsets, fill=ISENT):
    """int32 [N, H W]: the first row of every branch at its root slot, ``fill`` everywhere else"""
    N, H, W = blabels.shape
    out = np.full((N, H * W), fill, np.int64)
    j = 0
    for n in range(N):
        for lab in np.unique(blabels[n][blabels[n] != 0]):
            out[n, lab - 1] = offsets[j]
            j += 1
    assert j == len(chain)
    return out.astype(np.int32)


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", list(PC.cases()))
def test_rank_and_diag_equal_the_restatement(name):
    """every case of branch_cases.cases() -- 1 x 1 up to 130 x 260 (3 x 3 tiles), seams, borders, strokes over a four-tile corner, noise at
    four densities, crack skeletons, all ones, all zeros -- and the serpentines of 16 964 pixels in 15 rounds and 4 322 in 13, the
    staircase, the pixel between two junctions, the rings on the corner of four tiles and the two planes in either order"""
    topo, bl, want_rank, want_diag, rounds = PC.expected(name)
    rank, diag, P, R = device_order(topo, bl)
    assert rank.dtype == np.int32 and np.array_equal(rank, want_rank), np.argwhere(rank != want_rank)[:5]
    assert np.array_equal(diag, want_diag), np.argwhere(diag != want_diag)[:5]
    assert R == (math.ceil(math.log2(P)) if P > 1 else 0) and rounds <= R <= PC.rounds_bound(max(P, 1))


@pytest.mark.parametrize("name", ["cracks", "noise_0.3", "corner_rings", "serpentine_66x130", "borders", "staircase", "zeros"])
@pytest.mark.parametrize("with_d2", [False, True])
def test_the_scattered_points_equal_the_restatement(name, with_d2):
    topo, bl, rank, diag, _ = PC.expected(name)
    d2 = BC.fake_d2(bl) if with_d2 else None
    chain, offsets, want = PC.polylines_of(bl, rank, diag, d2)
    got = device_points(bl, rank, diag, _offset_planes(bl, chain, offsets), len(want), d2)
    assert np.array_equal(got, want)


def test_two_runs_are_bit_equal():
    for name in ("noise_0.6", "cracks", "serpentine_130x260", "noise_130x260"):
        topo, bl = PC.expected(name)[:2]
        a, b = device_order(topo, bl), device_order(topo, bl)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_a_row_outside_the_table_is_not_written():
    """offsets that point past the table, and a P below the true count: wrong numbers, nothing outside an array"""
    from csbsr_amd import _lib as L
    lib = L.load()
    topo, bl, rank, diag, _ = PC.expected("cracks")
    chain, offsets, want = PC.polylines_of(bl, rank, diag)
    got = device_points(bl, rank, diag, _offset_planes(bl, chain, offsets + len(want) - 5), len(want))
    assert (got[:len(want) - 5] == ISENT).all()
    N, H, W = topo.shape
    t, b = _inp(topo, LINKED, torch.uint8, 2 * (W + 2)), _inp(bl, 1, torch.int32, 2 * (W + 2))
    P = 100                                                                          # of 2 033
    ww, work = _out(int(lib.csbsr_branch_order_work_bytes(P)) // 4)
    (wr, rk), (wd, dg) = _out(N * H * W), _out(N * H * W)
    L.call("csbsr_branch_order", _ptr(t), _ptr(b), N, H, W, P, _ptr(work), _ptr(rk), _ptr(dg), _stream())
    torch.cuda.synchronize()
    _margins_intact(ww, wr, wd)
    assert int((rk >= 0).sum()) <= P and bool(((rk >= -1) & (rk < H * W)).all())


# ------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    lib = L.load()
    topo = torch.full((64,), LINKED, dtype=torch.uint8, device=DEV)
    lab = torch.ones(64, dtype=torch.int32, device=DEV)
    count = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    work, rank, diag, points = (torch.full((n,), ISENT, dtype=torch.int32, device=DEV) for n in (4096, 64, 64, 256))
    st = _stream()
    order = lambda **k: ("csbsr_branch_order", k.get("topo", _ptr(topo)), k.get("bl", _ptr(lab)), k.get("N", 1), k.get("H", 8), k.get("W", 8),
                         k.get("P", 64), k.get("work", _ptr(work)), k.get("rank", _ptr(rank)), k.get("diag", _ptr(diag)), st)
    scatter = lambda **k: ("csbsr_branch_scatter", k.get("bl", _ptr(lab)), k.get("rank", _ptr(rank)), k.get("diag", _ptr(diag)), k.get("d2", None),
                           k.get("off", _ptr(lab)), k.get("N", 1), k.get("H", 8), k.get("W", 8), k.get("rows", 64), k.get("points", _ptr(points)), st)
    calls = []
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(H=-8), dict(W=-8), dict(H=8193), dict(W=8193), dict(N=65536)):
        calls += [order(**bad), scatter(**bad), ("csbsr_branch_count", _ptr(topo), bad.get("N", 1), bad.get("H", 8), bad.get("W", 8), _ptr(count), st)]
    calls += [order(P=-1), order(P=(1 << 28) + 1), scatter(rows=-1)]
    calls += [order(**{k: None}) for k in ("topo", "bl", "work", "rank", "diag")] + [scatter(**{k: None}) for k in ("bl", "rank", "diag", "off", "points")]
    calls += [("csbsr_branch_count", None, 1, 8, 8, _ptr(count), st), ("csbsr_branch_count", _ptr(topo), 1, 8, 8, None, st)]
    # an output that is also an input or the other output
    calls += [order(rank=_ptr(diag)), order(rank=_ptr(lab)), order(diag=_ptr(lab)), order(rank=_ptr(work)), order(diag=_ptr(work)), order(work=_ptr(lab)),
              order(rank=_ptr(topo)), scatter(points=_ptr(lab)), scatter(points=_ptr(rank)), scatter(points=_ptr(diag)),
              scatter(d2=_ptr(points))]
    calls += [order(work=C.c_void_p(work.data_ptr() + 4)), scatter(points=C.c_void_p(points.data_ptr() + 4))]        # not 16-byte aligned
    for call in calls:
        with pytest.raises(L.CsbsrHipError):
            L.call(*call)
    assert int(lib.csbsr_branch_order_work_bytes(-1)) == 0 and int(lib.csbsr_branch_order_work_bytes((1 << 28) + 1)) == 0
    assert [int(lib.csbsr_branch_order_rounds(p)) for p in (0, 1, 2, 3, 4, 5, 4322, 16384, 16385)] == [0, 0, 1, 2, 2, 3, 13, 14, 15]
    torch.cuda.synchronize()
    assert int(count) == -7
    for t in (work, rank, diag, points):                                             # nothing ran: no output was written
        assert bool((t == ISENT).all())


# ------------------------------------------------------------------------------------------------ the Python surface
def test_order_branches_and_branch_polylines_surface():
    from csbsr_amd.utils import estimate_metrics as M
    for name in ("cracks", "serpentine_130x260", "corner_rings", "noise_0.3", "ones_between_zeros", "zeros", "swapped_ab", "swapped_ba"):
        topo_np, bl_np, rank_np, diag_np, rounds = PC.expected(name)
        N, H, W = topo_np.shape
        topo = torch.from_numpy(topo_np).to(DEV)
        bl = M.label_branches(topo)
        assert np.array_equal(bl.cpu().numpy(), bl_np)
        rank, diag, R = M.order_branches(bl, topo, return_rounds=True)
        P = int((bl_np != 0).sum())
        assert type(R) is int and rounds <= R <= PC.rounds_bound(max(P, 1))
        for got, want in ((rank, rank_np), (diag, diag_np)):
            assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (N, H, W) and np.array_equal(got.cpu().numpy(), want)
        again = M.order_branches(bl, torch.from_numpy(topo_np))                      # a CPU topo; two results without return_rounds
        assert len(again) == 2 and torch.equal(again[0], rank) and torch.equal(again[1], diag)
        d2_np = BC.fake_d2(bl_np)
        for d2 in (None, d2_np):
            chain, offsets, points = M.branch_polylines(bl, rank, diag, None if d2 is None else torch.from_numpy(d2).to(DEV))
            want = PC.polylines_of(bl_np, rank_np, diag_np, d2)
            assert chain.is_cuda and chain.dtype == torch.bool and offsets.dtype == torch.int64 and points.dtype == torch.int32
            for g, w in zip((chain, offsets, points), want):
                assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w)
        rows = M.branch_table(bl, topo).cpu().numpy()                                # the rows are those of branch_table
        assert len(rows) == len(want[0]) and np.array_equal(np.diff(want[1]), np.where(want[0], rows[:, 3], 0))
    topo = torch.from_numpy(PC.expected("cracks")[0]).to(DEV)
    bl = M.label_branches(topo)
    rank, diag = M.order_branches(bl, topo)
    for bad in ((bl, topo[:, :-1]), (bl, topo.to(torch.int32)), (bl.to(torch.int64), topo), (bl.cpu(), topo), (bl[0], topo[0])):
        with pytest.raises(ValueError):
            M.order_branches(*bad)
    for bad in ((bl, rank[:, :-1], diag), (bl, rank, diag.to(torch.int64)), (bl.cpu(), rank, diag), (bl, rank, diag, rank.to(torch.float32))):
        with pytest.raises(ValueError):
            M.branch_polylines(*bad)


# ------------------------------------------------------------------------------------------------ the driver
POLYLINE_KEYS = {"n_chains", "unordered_branch_px", "rank_map"}
POLYLINE_DICT_KEYS = {"chain", "start", "stop", "arc_px", "chord_px", "tortuosity", "direction_deg", "points"}


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


def _check_polyline_keys(g, wide):
    """the new keys of one yielded dict against the restatement on the returned branch_map and topology_map; returns the ordered pixels"""
    topo, bl = g["topology_map"].cpu().numpy(), g["branch_map"].cpu().numpy()
    rank, diag, _ = PC.jump_form(topo, bl)
    assert g["rank_map"].is_cuda and g["rank_map"].dtype == torch.int32 and np.array_equal(g["rank_map"].cpu().numpy(), rank)
    d2 = g["width_d2"].cpu().numpy() if wide else None
    want = PC.polyline_dicts(topo, bl, rank, diag, d2)
    assert len(want) == len(g["branches"]) == g["n_branches"]
    for b, w in zip(g["branches"], want):
        assert POLYLINE_DICT_KEYS <= set(b) and ("width_profile_px" in b) == wide
        for key in ("chain", "start", "stop", "arc_px", "chord_px", "tortuosity", "direction_deg"):
            assert b[key] == w[key] and type(b[key]) is type(w[key]), key
        assert isinstance(b["points"], np.ndarray) and b["points"].dtype == np.int32 and np.array_equal(b["points"], w["points"])
        assert b["points"].shape == (b["px"] if b["chain"] else 0, 2)
        if b["chain"]:
            assert (b["y"], b["x"]) == min(map(tuple, b["points"].tolist())) and b["arc_px"] <= b["length_geodesic_px"]
        if wide:
            assert b["width_profile_px"].dtype == np.float64 and np.array_equal(b["width_profile_px"], w["width_profile_px"])
            if b["chain"]:
                assert b["width_profile_px"].max() == b["max_width_px"]
    assert g["n_chains"] == sum(w["chain"] for w in want) and type(g["n_chains"]) is int
    assert g["unordered_branch_px"] == int(((bl != 0) & (rank < 0)).sum()) and type(g["unordered_branch_px"]) is int
    return int((rank >= 0).sum())


def test_predict_dataset_with_polylines(tmp_path):
    """test_predict_dataset_with_branches' two images (stitched maps of 64 x 96 and 84 x 68), with the polylines of the skeleton the call
    reports: whole, kept with min_crack_px, pruned with prune_spur_px, and with the width profile of width_radius"""
    import eval_io_cases as EC
    import predict_cases as PC2
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd import inference as I
    predict_dataset = I.predict_dataset
    images = PC2.make_images(PC2.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t, k, r, Lp = 0.4, 5, 64, 6
    base = dict(measure_threshold=t, topology=True, branches=True)
    total = 0
    for batch_patches in (16, 4):                                                    # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        options = {"whole": dict(), "kept": dict(min_crack_px=k), "width": dict(width_radius=r), "pruned": dict(prune_spur_px=Lp),
                   "all": dict(min_crack_px=k, width_radius=r, prune_spur_px=Lp)}
        for tag, opt in options.items():
            on_dir, off_dir = tmp_path / f"{batch_patches}_{tag}_on", tmp_path / f"{batch_patches}_{tag}_off"
            on = list(predict_dataset(EC.stub_model, ld, save_dir=str(on_dir), polylines=True, **base, **opt))
            off = list(predict_dataset(EC.stub_model, ld, save_dir=str(off_dir), **base, **opt))
            wide = "width_radius" in opt
            for g, o in zip(on, off):
                assert set(g) == set(o) | POLYLINE_KEYS
                total += _check_polyline_keys(g, wide)
                # every key of the call without the option is bit-equal
                new = POLYLINE_DICT_KEYS | ({"width_profile_px"} if wide else set())
                assert [{q: v for q, v in b.items() if q not in new} for b in g["branches"]] == o["branches"]
                assert all(set(b) == set(c) | new for b, c in zip(g["branches"], o["branches"]))
                _same({q: v for q, v in g.items() if q not in POLYLINE_KEYS | {"branches"}}, {q: v for q, v in o.items() if q != "branches"})
            fa, fb = _files(on_dir), _files(off_dir)
            assert set(fa) == set(fb) | {"crack_polylines.csv"} and all(fa[n] == fb[n] for n in fb)      # and so is every file
            back = dict(I.read_crack_polylines(str(on_dir / "crack_polylines.csv")))
            for g in on:
                kept = [(j, b) for j, b in enumerate(g["branches"]) if b["chain"]]
                got = back.get(g["name"], [])
                assert [d["branch"] for d in got] == [j for j, _ in kept]
                for (j, b), d in zip(kept, got):
                    assert np.array_equal(d["points"], b["points"]) and d["s_px"][-1] == b["arc_px"]
                    assert ("width_px" in d) == wide and (not wide or np.array_equal(d["width_px"], b["width_profile_px"]))
            header = SC.read_csv(str(on_dir / "crack_polylines.csv"))[0]
            assert header == I.POLYLINE_CSV_COLUMNS + (I.POLYLINE_CSV_OPTIONAL if wide else [])
    assert total > 200, "the maps have ordered pixels"
    # polylines=False is the call without the argument: the same keys, values and files
    for kwargs in (dict(), dict(measure_threshold=t), dict(**base), dict(min_crack_px=k, width_radius=5, **base)):
        tag = "_".join(sorted(kwargs)) or "plain"
        off = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_off"), polylines=False, **kwargs))
        none = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_none"), **kwargs))
        assert len(off) == len(none) == 2
        for x, y in zip(off, none):
            assert not (set(x) & POLYLINE_KEYS) and not any(set(b) & POLYLINE_DICT_KEYS for b in x.get("branches", []))
            bx, by = x.pop("branches", None), y.pop("branches", None)
            assert bx == by
            _same(x, y)
        fa, fb = _files(tmp_path / f"{tag}_off"), _files(tmp_path / f"{tag}_none")
        assert fa == fb and not any("polylines" in n for n in fa)
    # an all-zero map has no polyline
    zero = lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs))
    for kwargs in (dict(), dict(min_crack_px=k), dict(width_radius=5, prune_spur_px=3)):
        g = next(predict_dataset(zero, ld, polylines=True, **base, **kwargs))
        assert (g["n_chains"], g["unordered_branch_px"], g["branches"]) == (0, 0, []) and bool((g["rank_map"] == -1).all())
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(polylines=True), dict(measure_threshold=t, topology=True, polylines=True),
                   dict(polylines=1, **base), dict(polylines=None, **base), dict(polylines="True", **base)):
        with pytest.raises(ValueError):
            next(predict_dataset(model, ld, **kwargs))
