"""csrc/simplify.hip and its drivers on the device: keep and vcount are integers and are asked for exactly, at every row and for every
tolerance, against the NumPy restatement of tests/simplify_cases.py (whose own properties tests/test_simplify_cpu.py holds).

Through the C ABI the offsets sit between values far outside the table and the points between rows of far-away coordinates, every output
inside a sentinel-filled allocation whose margins are checked, and ``work`` is sentinel-filled too: nothing may depend on what it held."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import simplify_cases as SV

pytestmark = pytest.mark.gpu

PAD = 64
ISENT = 0x5A5A5A5A
BSENT = 0x5A
DEV = torch.device("cuda", 0)


def _ptr(t):
    """the address of the view's first element, also where the view is empty (its place inside the padded allocation)"""
    return C.c_void_p(t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _inp(x, fill, dtype):
    x = torch.from_numpy(np.ascontiguousarray(x)).to(dtype).reshape(-1)
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


def device_simplify(offsets, points, tol_q):
    """(keep uint8 [P], vcount int32 [M]) of csbsr_polyline_simplify through the C ABI"""
    from csbsr_amd import _lib as L
    lib = L.load()
    M, P = len(offsets) - 1, len(points)
    off = _inp(offsets, 1 << 40, torch.int64)
    pts = _inp(points, 7777, torch.int32)
    need = int(lib.csbsr_polyline_simplify_work_bytes(M, P))
    assert need >= 16 and need % 4 == 0
    ww, work = _out(need // 4)
    (wk, keep), (wv, vcount) = _out(P, torch.uint8), _out(M)
    L.call("csbsr_polyline_simplify", _ptr(off), _ptr(pts), M, P, tol_q, _ptr(work), _ptr(keep), _ptr(vcount), _stream())
    torch.cuda.synchronize()
    _margins_intact(ww, wk, wv)
    return keep.cpu().numpy(), vcount.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", list(SV.cases()))
def test_keep_and_vcount_equal_the_restatement(name):
    """the spans of the polyline cases -- thousands of chains of 1 to 3 points, crack skeletons, rings, ONE chain of 16 964 points -- and the
    synthetic tables: spans of 0 to 3 rows, collinear runs, digital lines, equal keys, the growing saw (a round per point), 2^58 products,
    repeated points, random walks one row short of, at and one row past every route limit, and two tables in either order"""
    offsets, points = SV.cases()[name]
    for tol_q in SV.TOL_Q:
        keep, vcount = device_simplify(offsets, points, tol_q)
        want_keep, want_vcount = SV.expected(name, tol_q)
        assert keep.dtype == np.uint8 and np.array_equal(keep, want_keep), (tol_q, np.nonzero(keep != want_keep)[0][:8])
        assert vcount.dtype == np.int32 and np.array_equal(vcount, want_vcount), (tol_q, np.nonzero(vcount != want_vcount)[0][:8])


def test_two_runs_are_bit_equal():
    for name in ("noise_0.3", "cracks", "route_seams", "serpentine_66x130"):
        offsets, points = SV.cases()[name]
        a, b = device_simplify(offsets, points, 4), device_simplify(offsets, points, 4)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _cut(yx, a, b, tol_q, limit, out):
    """the segments of the recursion's upper levels, down to pieces of at most ``limit`` rows: each is a problem of its own"""
    if b - a + 1 > limit:
        key, c2 = SV.keys_of(yx[a], yx[b], yx[a + 1:b])
        i = int(np.argmax(key))
        if SV.splits(key[i], c2, tol_q):
            _cut(yx, a, a + 1 + i, tol_q, limit, out)
            _cut(yx, a + 1 + i, b, tol_q, limit, out)
            return
    out.append((a, b))


def test_the_route_does_not_matter():
    """a walk as one span (a workgroup's, its state in LDS or in work) and as the pieces the recursion's upper levels cut it into, a wave each"""
    from csbsr_amd.utils import estimate_metrics as M
    offsets, points = SV.cases()["route_seams"]
    assert tuple(np.diff(offsets)[[1, 4]]) == M.SIMPLIFY_ROUTE_LIMITS
    keep, vcount = device_simplify(offsets, points, 4)
    for j in (1, 3, 5):                                                              # 64 rows: a wave; 2047: LDS; 2049: work
        o0, o1 = int(offsets[j]), int(offsets[j + 1])
        pieces = []
        _cut(points[o0:o1, :2].astype(np.int64), 0, o1 - o0 - 1, 4, 32, pieces)
        spans = [points[o0 + a:o0 + b + 1] for a, b in pieces]
        assert len(spans) > 1 and max(len(s) for s in spans) <= M.SIMPLIFY_ROUTE_LIMITS[0]
        off2 = np.concatenate([np.zeros(1, np.int64), np.cumsum([len(s) for s in spans])])
        k2, v2 = device_simplify(off2, np.concatenate(spans), 4)
        want = [keep[o0 + a:o0 + b + 1] for a, b in pieces]
        assert np.array_equal(k2, np.concatenate(want)) and int(v2.sum()) == int(vcount[j]) + len(spans) - 1


def test_bad_offsets_write_nothing_outside():
    """descending offsets and offsets outside 0 .. P: those spans are skipped -- vcount 0, their rows 0 -- and nothing is written outside"""
    offsets, points = SV.cases()["cracks"]
    P = len(points)
    bad = offsets.copy()
    bad[5], bad[10], bad[20], bad[30], bad[40], bad[-1] = -3, P + 7, 1 << 40, -(1 << 62), (1 << 62), P + 1
    for tol_q in (0, 4):
        keep, vcount = device_simplify(bad, points, tol_q)
        want_keep, want_vcount = SV.simplify_table(bad, points, tol_q)
        assert np.array_equal(keep, want_keep) and np.array_equal(vcount, want_vcount)
        assert vcount[[4, 5, 9, 10, 19, 20, 29, 30, 39, 40, len(bad) - 2]].tolist() == [0] * 11 and int(vcount.sum()) > 0
    # every offset bad: nothing is kept
    keep, vcount = device_simplify(offsets[::-1].copy() + 1, points, 4)
    assert not keep.any() and not vcount.any()


def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    from csbsr_amd.utils import estimate_metrics as M
    lib = L.load()
    off = torch.tensor([0, 3, 8], dtype=torch.int64, device=DEV)
    pts = torch.zeros(8, 4, dtype=torch.int32, device=DEV)
    work, vcount = (torch.full((n,), ISENT, dtype=torch.int32, device=DEV) for n in (4096, 64))
    keep = torch.full((64,), BSENT, dtype=torch.uint8, device=DEV)
    st = _stream()
    call = lambda **k: ("csbsr_polyline_simplify", k.get("off", _ptr(off)), k.get("pts", _ptr(pts)), k.get("M", 2), k.get("P", 8), k.get("tol_q", 4),
                        k.get("work", _ptr(work)), k.get("keep", _ptr(keep)), k.get("vcount", _ptr(vcount)), st)
    calls = [call(**{k: None}) for k in ("off", "pts", "work", "keep", "vcount")]
    calls += [call(M=-1), call(M=(1 << 28) + 1), call(P=-1), call(P=(1 << 28) + 1), call(tol_q=-1), call(tol_q=65)]
    # an output that is an input, the other output or work
    calls += [call(keep=_ptr(off)), call(keep=_ptr(pts)), call(keep=_ptr(work)), call(keep=_ptr(vcount)), call(vcount=_ptr(off)), call(vcount=_ptr(pts)),
              call(vcount=_ptr(work)), call(vcount=_ptr(keep)), call(work=_ptr(off)), call(work=_ptr(pts))]
    calls += [call(work=C.c_void_p(work.data_ptr() + 4)), call(work=C.c_void_p(work.data_ptr() + 8)), call(pts=C.c_void_p(pts.data_ptr() + 8))]
    for c in calls:
        with pytest.raises(L.CsbsrHipError):
            L.call(*c)
    torch.cuda.synchronize()
    for t, sent in ((work, ISENT), (vcount, ISENT), (keep, BSENT)):                  # nothing ran: no output was written
        assert bool((t == sent).all())
    assert bool((pts == 0).all()) and off.tolist() == [0, 3, 8]
    wb = lib.csbsr_polyline_simplify_work_bytes
    assert [int(wb(*a)) for a in ((-1, 0), (0, -1), ((1 << 28) + 1, 0), (0, (1 << 28) + 1))] == [0] * 4
    assert int(wb(0, 0)) > 0 and int(wb(1 << 28, 1 << 28)) >= 20 << 28 and int(wb(3, 1000)) % 16 == 0
    assert int(lib.csbsr_simplify_max_tol_q()) == 64 == int(4 * M.SIMPLIFY_MAX_PX)
    a, b = C.c_int32(), C.c_int32()
    L.call("csbsr_simplify_route_limits", C.byref(a), C.byref(b))
    assert (a.value, b.value) == M.SIMPLIFY_ROUTE_LIMITS == SV.ROUTE_LIMITS


# ------------------------------------------------------------------------------------------------ the Python surface
def test_simplify_polylines_surface(monkeypatch):
    from csbsr_amd import _lib as L
    from csbsr_amd.utils import estimate_metrics as M
    for name in ("cracks", "noise_0.6", "serpentine_66x130", "route_seams", "tiny_spans", "swapped_ab"):
        off_np, pts_np = SV.cases()[name]
        off, pts = torch.from_numpy(off_np).to(DEV), torch.from_numpy(pts_np).to(DEV)
        for px in (0, 0.5, 1.0, 2, 16.0):
            keep, voffsets, vindex = M.simplify_polylines(off, pts, px)
            want_keep, want_vcount = SV.expected(name, int(px * 4))
            assert keep.is_cuda and keep.dtype == torch.uint8 and tuple(keep.shape) == (len(pts_np),) and np.array_equal(keep.cpu().numpy(), want_keep)
            assert voffsets.is_cuda and voffsets.dtype == torch.int64 and tuple(voffsets.shape) == (len(off_np),)
            assert np.array_equal(voffsets.cpu().numpy(), np.concatenate([[0], np.cumsum(want_vcount)]))
            assert vindex.is_cuda and vindex.dtype == torch.int32 and np.array_equal(vindex.cpu().numpy(), np.nonzero(want_keep)[0])
            assert torch.equal(pts[vindex.long()], pts[keep.bool()])
    # the table of branch_polylines itself
    import polyline_cases as PC
    topo = torch.from_numpy(PC.expected("cracks")[0]).to(DEV)
    bl = M.label_branches(topo)
    _, off, pts = M.branch_polylines(bl, *M.order_branches(bl, topo))
    assert np.array_equal(M.simplify_polylines(off, pts, 0.5)[0].cpu().numpy(), SV.expected("cracks", 2)[0])
    for bad in ((off.to(torch.int32), pts, 1.0), (off, pts.to(torch.int64), 1.0), (off, pts[:, :3], 1.0), (off.view(1, -1), pts, 1.0), (off[:0], pts, 1.0),
                (off.cpu(), pts, 1.0), (off, pts.cpu(), 1.0), (off.cpu().numpy(), pts, 1.0), (off, pts, 0.3), (off, pts, True), (off, pts, 16.25),
                (off, pts.view(-1), 1.0)):
        with pytest.raises(ValueError):
            M.simplify_polylines(*bad)
    # M == 0 and P == 0 run without a launch
    monkeypatch.setattr(L, "call", lambda *a, **k: pytest.fail("a launch"))
    empty = M.simplify_polylines(off[:1], pts[:0], 1.0)
    assert [tuple(t.shape) for t in empty] == [(0,), (1,), (0,)] and [t.dtype for t in empty] == [torch.uint8, torch.int64, torch.int32]
    keep, voffsets, vindex = M.simplify_polylines(torch.zeros(4, dtype=torch.int64, device=DEV), pts[:0], 1.0)
    assert tuple(keep.shape) == (0,) and voffsets.tolist() == [0] * 4 and tuple(vindex.shape) == (0,) and all(t.is_cuda for t in (keep, voffsets, vindex))
    keep, voffsets, vindex = M.simplify_polylines(off[:1], pts, 1.0)
    assert tuple(keep.shape) == (len(pts),) and not bool(keep.any()) and voffsets.tolist() == [0] and tuple(vindex.shape) == (0,)


# ------------------------------------------------------------------------------------------------ the driver
VERTEX_KEYS = {"n_vertices", "length_simplified_px"}
VERTEX_DICT_KEYS = {"vertices", "vertex_index", "length_simplified_px"}


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


def _check_vertex_keys(g, tol_q, wide):
    """the new keys of one yielded dict against the restatement applied to the returned points; returns (chains, vertices).  The lengths are
    fp64 sums of v - 1 (closed: v) non-negative terms: two orders of summation differ by at most 2 v 2^-53 of the sum."""
    want, nv, _ = SV.vertex_dicts(g["branches"], tol_q, widths=wide)
    new = VERTEX_DICT_KEYS | ({"vertex_width_px"} if wide else set())
    for b, w in zip(g["branches"], want):
        assert new <= set(b) and ("vertex_width_px" in b) == wide
        assert isinstance(b["vertices"], np.ndarray) and b["vertices"].dtype == np.int32 and np.array_equal(b["vertices"], w["vertices"])
        assert b["vertex_index"].dtype == np.int32 and np.array_equal(b["vertex_index"], w["vertex_index"])
        assert b["vertices"].shape == (len(b["vertex_index"]), 2) and np.array_equal(b["points"][b["vertex_index"]], b["vertices"])
        if b["chain"]:
            v = len(b["vertices"])
            assert 1 <= v <= b["px"] and (v >= 2 or b["px"] == 1) and tuple(b["vertices"][0]) == b["start"] and tuple(b["vertices"][-1]) == b["stop"]
            assert type(b["length_simplified_px"]) is float
            assert abs(b["length_simplified_px"] - w["length_simplified_px"]) <= 2 * v * 2.0 ** -53 * w["length_simplified_px"]
            if b["tortuosity"] is not None:                                          # an open chain: no shorter than its chord, no longer than its arc
                assert b["chord_px"] <= b["length_simplified_px"] * (1 + 1e-12) and b["length_simplified_px"] <= b["arc_px"] * (1 + 1e-12)
        else:
            assert b["length_simplified_px"] is None and b["vertices"].shape == (0, 2) and b["vertex_index"].shape == (0,)
        if wide:
            assert b["vertex_width_px"].dtype == np.float64 and np.array_equal(b["vertex_width_px"], b["width_profile_px"][b["vertex_index"]])
    chains = [b for b in g["branches"] if b["chain"]]
    assert g["n_vertices"] == nv == sum(len(b["vertices"]) for b in chains) and type(g["n_vertices"]) is int
    assert g["length_simplified_px"] == sum([b["length_simplified_px"] for b in chains], 0.0) and type(g["length_simplified_px"]) is float
    return len(chains), nv


def test_predict_dataset_with_simplify_px(tmp_path):
    """test_predict_dataset_with_polylines' two images (stitched maps of 64 x 96 and 84 x 68) and option sets, with the simplified polylines
    of the polylines the call reports: whole, kept with min_crack_px, pruned with prune_spur_px, and with the widths of width_radius"""
    import eval_io_cases as EC
    import predict_cases as PC2
    import skeleton_cases as SC
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd import inference as I
    predict_dataset = I.predict_dataset
    images = PC2.make_images(PC2.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t, k, r, Lp = 0.4, 5, 64, 6
    base = dict(measure_threshold=t, topology=True, branches=True, polylines=True)
    vertices = points = 0
    for batch_patches in (16, 4):                                                    # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        options = {"whole": (1.0, dict()), "kept": (0.5, dict(min_crack_px=k)), "width": (2, dict(width_radius=r)), "pruned": (0, dict(prune_spur_px=Lp)),
                   "all": (0.25, dict(min_crack_px=k, width_radius=r, prune_spur_px=Lp))}
        for tag, (px, opt) in options.items():
            on_dir, off_dir = tmp_path / f"{batch_patches}_{tag}_on", tmp_path / f"{batch_patches}_{tag}_off"
            on = list(predict_dataset(EC.stub_model, ld, save_dir=str(on_dir), simplify_px=px, **base, **opt))
            off = list(predict_dataset(EC.stub_model, ld, save_dir=str(off_dir), **base, **opt))
            wide = "width_radius" in opt
            new = VERTEX_DICT_KEYS | ({"vertex_width_px"} if wide else set())
            chains = 0
            for g, o in zip(on, off):
                assert set(g) == set(o) | VERTEX_KEYS
                c, v = _check_vertex_keys(g, int(px * 4), wide)
                chains, vertices, points = chains + c, vertices + v, points + sum(len(b["points"]) for b in g["branches"])
                # every key of the call without the option is bit-equal
                assert all(set(b) == set(c) | new for b, c in zip(g["branches"], o["branches"]))
                _same({q: v for q, v in g.items() if q not in VERTEX_KEYS | {"branches"}}, {q: v for q, v in o.items() if q != "branches"})
                _same_value([{q: v for q, v in b.items() if q not in new} for b in g["branches"]], o["branches"], "branches")
            fa, fb = _files(on_dir), _files(off_dir)
            assert set(fa) == set(fb) | {"crack_vertices.csv", "crack_polylines.geojson"} and all(fa[n] == fb[n] for n in fb)      # and so is every file
            back = dict(I.read_crack_vertices(str(on_dir / "crack_vertices.csv")))
            for g in on:
                kept = [(j, b) for j, b in enumerate(g["branches"]) if b["chain"]]
                got = back.get(g["name"], [])
                assert [d["branch"] for d in got] == [j for j, _ in kept]
                for (j, b), d in zip(kept, got):
                    assert np.array_equal(d["vertices"], b["vertices"]) and np.array_equal(d["vertex_index"], b["vertex_index"])
                    assert ("width_px" in d) == wide and (not wide or np.array_equal(d["width_px"], b["vertex_width_px"]))
            assert SC.read_csv(str(on_dir / "crack_vertices.csv"))[0] == I.VERTEX_CSV_COLUMNS + (I.VERTEX_CSV_OPTIONAL if wide else [])
            doc = json.loads(fa["crack_polylines.geojson"].decode())
            assert doc["type"] == "FeatureCollection" and len(doc["features"]) == chains > 0
            at = iter(doc["features"])
            for g in on:
                for j, b in enumerate(g["branches"]):
                    if not b["chain"]:
                        continue
                    f = next(at)
                    p, xy = f["properties"], [[x, y] for y, x in b["vertices"].tolist()]
                    assert (p["name"], p["branch"], p["kind"], p["px"], p["n_vertices"]) == (g["name"], j, b["kind"], b["px"], len(xy))
                    assert p["length_simplified_px"] == b["length_simplified_px"] and p["arc_px"] == b["arc_px"]
                    assert p["closed"] is (sum(b["links"]) - b["attach"] == b["px"])
                    assert ("crack" in p) == ("min_crack_px" in opt) and ("max_width_px" in p) == wide == ("min_width_px" in p)
                    want = {"type": "Point", "coordinates": xy[0]} if len(xy) == 1 else {"type": "LineString", "coordinates": xy + (xy[:1] if p["closed"] else [])}
                    assert f["geometry"] == want
    assert points > vertices > 0, "the maps have polylines, and the option simplifies them"
    # simplify_px=None is the call without the argument: the same keys, values and files
    for kwargs in (dict(), dict(measure_threshold=t), dict(**base), dict(min_crack_px=k, width_radius=5, **base)):
        tag = "_".join(sorted(kwargs)) or "plain"
        none = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_none"), simplify_px=None, **kwargs))
        off = list(predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / f"{tag}_off"), **kwargs))
        assert len(off) == len(none) == 2
        for x, y in zip(none, off):
            assert not (set(x) & VERTEX_KEYS) and not any(set(b) & (VERTEX_DICT_KEYS | {"vertex_width_px"}) for b in x.get("branches", []))
            _same(x, y)
        fa, fb = _files(tmp_path / f"{tag}_none"), _files(tmp_path / f"{tag}_off")
        assert fa == fb and not any("vertices" in n or "geojson" in n for n in fa)
    # an all-zero map has no vertex
    zero = lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs))
    for kwargs in (dict(), dict(min_crack_px=k), dict(width_radius=5, prune_spur_px=3)):
        g = next(predict_dataset(zero, ld, simplify_px=1.0, **base, **kwargs))
        assert (g["n_vertices"], g["length_simplified_px"], g["branches"]) == (0, 0.0, [])
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(simplify_px=1.0), dict(simplify_px=1.0, measure_threshold=t, topology=True, branches=True),
                   dict(simplify_px=1.0, measure_threshold=t, topology=True, branches=True, polylines=False), dict(simplify_px=0.3, **base),
                   dict(simplify_px=True, **base), dict(simplify_px=-0.25, **base), dict(simplify_px=16.25, **base), dict(simplify_px="1", **base)):
        with pytest.raises(ValueError):
            next(predict_dataset(model, ld, **kwargs))
