"""The NumPy restatement of the polyline simplification (tests/simplify_cases.py): the recursion against the rounds form on every case and
tolerance, the ends, an independent fp64 distance bound on every dropped point, digital lines, the tie rule, the host helpers of
utils/estimate_metrics.py, the header against the binding, and the CSV / GeoJSON writers and readers of inference.py.  Nothing here needs a
GPU."""
import inspect
import json
import math
import os
import re

import numpy as np
import pytest

import branch_cases as BC
import polyline_cases as PC
import simplify_cases as SV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(SV.cases()))
def test_the_recursion_and_the_rounds_form_agree(name):
    offsets, points = SV.cases()[name]
    assert offsets.dtype == np.int64 and points.dtype == np.int32 and points.shape == (int(offsets[-1]), 4)
    for tol_q in SV.TOL_Q:
        keep, vcount = SV.expected(name, tol_q)
        k2, v2 = SV.simplify_table(offsets, points, tol_q, form=SV.simplify_stack)
        assert np.array_equal(keep, k2) and np.array_equal(vcount, v2)
        assert keep.dtype == np.uint8 and vcount.dtype == np.int32 and int(keep.sum()) == int(vcount.sum())
        n = np.diff(offsets)
        assert np.array_equal(vcount[n <= 2], n[n <= 2]) and (vcount[n > 2] >= 2).all() and (vcount <= n).all()
        some = n > 0
        assert keep[offsets[:-1][some]].all() and keep[offsets[1:][some] - 1].all()   # the first and the last row of every span


@pytest.mark.parametrize("name", ["cracks", "corner_rings", "staircase", "digital_lines", "zigzag_tie", "saw_60", "random_corners", "repeated_points",
                                  "route_seams"])
def test_every_dropped_point_is_within_the_tolerance(name):
    """an independent fp64 distance to the segment between the kept neighbours: tol + 1e-9 bounds it at every dropped point"""
    offsets, points = SV.cases()[name]
    for tol_q in SV.TOL_Q:
        keep = SV.expected(name, tol_q)[0]
        worst = 0.0
        for o0, o1 in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
            kept = o0 + np.nonzero(keep[o0:o1])[0]
            for a, b in zip(kept[:-1].tolist(), kept[1:].tolist()):
                for r in range(a + 1, b):
                    worst = max(worst, SV.segment_distance(points[a, :2], points[b, :2], points[r, :2]))
        assert worst <= tol_q / 4 + 1e-9, (tol_q, worst)


def test_digital_lines_collapse_to_their_ends_from_half_a_pixel():
    offsets, points = SV.cases()["digital_lines"]
    assert np.diff(offsets).tolist() == [51] * len(SV.LINE_SLOPES)
    for tol_q in SV.TOL_Q:
        vcount = SV.expected("digital_lines", tol_q)[1]
        if tol_q >= 2:
            assert vcount.tolist() == [2] * len(SV.LINE_SLOPES)
    quarter = SV.expected("digital_lines", 1)[1].tolist()
    assert quarter[0] == 2 and quarter[-1] == 2 and min(quarter[1:-1]) > 2           # at 0.25 px a digital line does not collapse
    # the Euclidean length of the two ends is the true length of the line
    from csbsr_amd.utils import estimate_metrics as M
    for j, num in enumerate(SV.LINE_SLOPES):
        pts = points[offsets[j]:offsets[j + 1], :2]
        keep = SV.expected("digital_lines", 2)[0][offsets[j]:offsets[j + 1]]
        assert M.polyline_length(pts[keep != 0]) == math.hypot(50, num)


def test_the_smaller_row_wins_among_equal_keys():
    """ZIGZAG: rows 1 and 3 are equally far from the chord; row 1 is kept first, then rows 2 and 3 are equally far (1.79 px) from the
    segment 1 -> 4.  At 2 px neither stays -- had row 3 won the first tie, the result would be rows 0, 3, 4."""
    a, b = np.array(SV.ZIGZAG[0]), np.array(SV.ZIGZAG[-1])
    key, c2 = SV.keys_of(a, b, np.array(SV.ZIGZAG[1:-1]))
    assert key[0] == key[2] > key[1] and c2 == 64
    key, _ = SV.keys_of(SV.ZIGZAG[1], SV.ZIGZAG[4], np.array(SV.ZIGZAG[2:4]))
    assert key[0] == key[1]
    for form in (SV.simplify_stack, lambda p, t: SV.simplify_rounds(p, t)[0]):
        assert form(SV.ZIGZAG, 8).tolist() == [1, 1, 0, 0, 1]
        assert form(SV.ZIGZAG, 6).tolist() == [1, 1, 1, 1, 1]                        # at 1.5 px row 2 stays, and then row 3 is 3 px off
    assert SV.expected("zigzag_tie", 8)[0].tolist() == [1, 1, 0, 0, 1] + [1, 1, 0, 0, 1]


def test_the_depth_is_not_logarithmic():
    """the rounds a workgroup loops: a saw whose teeth grow gives up one tooth per round, the serpentine one turn"""
    # the restatement counts the rounds that examine a segment with an inner point: 58, one per inner point.  The kernel's loop makes one
    # more trip, which finds nothing to split -- the 59 rounds of a 60-point saw
    r60 = SV.simplify_rounds(SV.saw(60), 0)[1]
    assert r60 == 58 > 4 * math.ceil(math.log2(60))                                  # n - 2: every inner point in a round of its own
    assert SV.simplify_rounds(SV.saw(1500), 0)[1] == 1498
    off, pts = SV.cases()["serpentine_66x130"]
    n = np.diff(off)
    j = int(np.argmax(n))
    rs = SV.simplify_rounds(pts[off[j]:off[j + 1], :2], 2)[1]
    assert rs > 2 * math.ceil(math.log2(int(n[j]))), (rs, int(n[j]))
    off, pts = SV.cases()["serpentine_130x260"]
    assert np.diff(off).max() == 16964                                              # ONE chain, longer than the LDS route takes


def test_the_keys_stay_below_2_to_the_58():
    c = SV.SIDE - 1
    worst = 0
    for a, b, p in (((0, 0), (c, c), (0, c)), ((0, 0), (c, c), (c, 0)), ((0, 0), (0, 1), (c, c)), ((0, 0), (c, c), (c, c)), ((c, 0), (0, c), (c, c))):
        key, c2 = SV.keys_of(a, b, p)
        want = round(SV.segment_distance(a, b, p) ** 2 * (int(c2) if c2 else 1))
        assert abs(int(key) - want) <= 1e-9 * want
        worst = max(worst, int(key))
    assert 2 ** 50 < worst < 2 ** 58 and 16 * worst < 2 ** 63


def test_the_option_does_something_on_crack_skeletons():
    offsets, points = SV.cases()["cracks"]
    P = points.shape[0]
    counts = [int(SV.expected("cracks", t)[0].sum()) for t in (0, 2, 4, 8)]
    assert P > counts[0] > counts[1] > counts[2] > counts[3] >= 2 * int((np.diff(offsets) >= 2).sum())
    # the case tables the GPU tests aim at the routes with
    n = np.diff(SV.cases()["route_seams"][0]).tolist()
    assert n == [L + d for L in SV.ROUTE_LIMITS for d in (-1, 0, 1)]
    assert np.diff(SV.cases()["noise_0.3"][0]).max() <= 64 and np.diff(SV.cases()["saw_1500"][0]).tolist() == [1500]
    ab, ba = SV.cases()["swapped_ab"], SV.cases()["swapped_ba"]
    na = SV.cases()["cracks"][1].shape[0]
    for t in (0, 4):
        ka, kb = SV.expected("swapped_ab", t)[0], SV.expected("swapped_ba", t)[0]
        assert np.array_equal(ka[:na], kb[-na:]) and np.array_equal(ka[na:], kb[:-na]) and np.array_equal(ka[:na], SV.expected("cracks", t)[0])


# ------------------------------------------------------------------------------------------------ the host helpers
def test_simplify_tolerance():
    from csbsr_amd.utils import estimate_metrics as M
    assert M.SIMPLIFY_MAX_PX == 16.0 and M.SIMPLIFY_ROUTE_LIMITS == SV.ROUTE_LIMITS and all(type(v) is int for v in M.SIMPLIFY_ROUTE_LIMITS)
    for px, q in ((0, 0), (0.0, 0), (0.25, 1), (0.5, 2), (1, 4), (1.0, 4), (1.75, 7), (2, 8), (16, 64), (16.0, 64), (np.float64(0.75), 3), (np.int64(3), 12),
                  (np.float32(1.5), 6)):
        assert M.simplify_tolerance(px) == q and type(M.simplify_tolerance(px)) is int
    for bad in (True, False, np.bool_(True), None, "1", [1], -0.25, -1, 16.25, 17, 0.1, 0.3, 1e-9, float("nan"), float("inf"), 1 + 2 ** -40, 1j):
        with pytest.raises(ValueError) as e:
            M.simplify_tolerance(bad, "simplify_px")
        assert "simplify_px" in str(e.value)


def test_polyline_length():
    from csbsr_amd.utils import estimate_metrics as M
    assert M.polyline_length(np.zeros((0, 2), np.int32)) == 0.0 and M.polyline_length([(3, 4)]) == 0.0 and M.polyline_length([(3, 4)], closed=True) == 0.0
    assert M.polyline_length([(0, 0), (3, 4)]) == 5.0 and M.polyline_length([(0, 0), (3, 4)], closed=True) == 10.0
    sq = [(0, 0), (0, 4), (4, 4), (4, 0)]
    assert M.polyline_length(sq) == 12.0 and M.polyline_length(sq, closed=True) == 16.0 and type(M.polyline_length(sq)) is float
    assert M.polyline_length(np.array([(0, 0, 5, 9), (1, 1, 6, 9)], np.int32)) == math.sqrt(2.0)       # rows of branch_polylines: y and x first
    import torch
    assert M.polyline_length(torch.tensor(sq)) == 12.0
    for bad in (np.array([1, 2, 3]), np.zeros((3, 1))):
        with pytest.raises(ValueError):
            M.polyline_length(bad)


def test_abi_matches_the_header():
    from csbsr_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    ctype = {"const int64_t*": L.vp, "const int32_t*": L.vp, "void*": L.vp, "uint8_t*": L.vp, "int32_t*": L.vp, "csbsr_stream_t": L.vp, "int32_t": L.i32}
    want = {"csbsr_polyline_simplify": ("int", 9), "csbsr_polyline_simplify_work_bytes": ("int64_t", 2), "csbsr_simplify_max_tol_q": ("int32_t", 0)}
    for name, (res, nargs) in want.items():
        decl = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl and decl.group(1) == res, f"{name} is not declared in include/csbsr_hip.h"
        text = decl.group(2).replace("\n", " ").strip()
        args = [] if text == "void" else [ctype[" ".join(a.split()[:-1])] for a in text.split(",")]
        r, sig = L.SIGNATURES[name]
        assert r is {"int": L.i32, "int32_t": L.i32, "int64_t": L.i64}[res] and sig == args and len(args) == nargs
    assert re.search(r"int\s+csbsr_simplify_route_limits\s*\(\s*int32_t\*\s*\w+\s*,\s*int32_t\*\s*\w+\s*\)\s*;", hdr)
    assert len(L.SIGNATURES["csbsr_simplify_route_limits"][1]) == 2
    assert "simplify.hip" in open(os.path.join(ROOT, "csbsr_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "csbsr_amd", "csrc", "simplify.hip")).read()       # the route limits are mirrored in Python
    limits = tuple(int(re.search(r"#define\s+%s\s+(\d+)" % k, src).group(1)) for k in ("SP_WAVE_MAX", "SP_LDS_MAX"))
    assert limits == SV.ROUTE_LIMITS and not re.search(r"\b(float|double)\b", re.sub(r"//[^\n]*", "", src))


def test_predict_dataset_takes_simplify_px_and_refuses_it_before_the_model_runs():
    from csbsr_amd.inference import predict_dataset
    assert inspect.signature(predict_dataset).parameters["simplify_px"].default is None
    model = lambda *a, **kw: pytest.fail("the model ran")
    base = dict(measure_threshold=0.4, topology=True, branches=True)
    for kwargs in (dict(simplify_px=1.0), dict(simplify_px=1.0, **base), dict(simplify_px=1.0, polylines=False, **base),
                   dict(simplify_px=0.3, polylines=True, **base), dict(simplify_px=True, polylines=True, **base),
                   dict(simplify_px=-1, polylines=True, **base), dict(simplify_px=16.25, polylines=True, **base),
                   dict(simplify_px="1", polylines=True, **base), dict(simplify_px=1.0, polylines=True, measure_threshold=0.4, topology=True)):
        with pytest.raises(ValueError):
            next(predict_dataset(model, None, **kwargs))


def test_the_device_entry_refuses_what_is_no_device_tensor():
    import torch
    from csbsr_amd.utils import estimate_metrics as M
    off, pts = torch.zeros(2, dtype=torch.int64), torch.zeros(3, 4, dtype=torch.int32)
    for bad in ((off, pts, 1.0), (off.numpy(), pts.numpy(), 1.0), (off, pts, 0.3)):
        with pytest.raises(ValueError):
            M.simplify_polylines(*bad)


# ------------------------------------------------------------------------------------------------ the files
def _hand_made(wide):
    """two images' branch lists with the polyline keys, made by hand: an open chain, a closed chain (as many inner links as pixels), a chain
    of one pixel and a branch that is no chain"""
    ring = [(2, 2), (2, 3), (2, 4), (3, 5), (4, 4), (4, 3), (4, 2), (3, 1)]
    run = [(7, x) for x in range(9)] + [(8, 9), (9, 10)]
    def branch(points, chain, kind, links, attach, crack):
        pts = np.array(points if chain else [], np.int32).reshape(-1, 2)
        d = dict(chain=chain, kind=kind, px=len(points), links=links, attach=attach, points=pts, crack=crack, arc_px=float(max(len(pts) - 1, 0)))
        if wide:
            d.update(width_profile_px=np.arange(len(pts), dtype=np.float64) / 4 + 1, max_width_px=9.0, min_width_px=1.0)
        return d
    a = [branch(run, True, "free", (8, 0, 2, 0), 0, 0), branch(ring, True, "ring", (2, 0, 3, 3), 0, 1), branch([(0, 9)], True, "isolated", (0, 0, 0, 0), 0, 2),
         branch([(5, 5), (5, 6), (6, 5), (6, 6)], False, "link", (2, 2, 1, 1), 2, 1)]
    b = [branch([(1, 1), (2, 2), (3, 3)], True, "free", (0, 0, 2, 0), 0, 0)]
    return [("a.png", a), ("b.png", b), ("empty.png", [])]


@pytest.mark.parametrize("wide", [False, True])
def test_the_vertex_keys_and_files_round_trip(tmp_path, wide):
    from csbsr_amd import inference as I
    rows = _hand_made(wide)
    for tol_q in (0, 2, 4):
        totals = []
        for _, branches in rows:
            points = np.concatenate([np.concatenate([b["points"], np.zeros_like(b["points"])], 1) for b in branches] + [np.zeros((0, 4), np.int32)])
            if wide:
                points[:, 3] = np.concatenate([np.round((b["width_profile_px"] + 1) ** 2 / 4) for b in branches] + [np.zeros(0)])
            keep = np.concatenate([SV.simplify_stack(b["points"], tol_q) for b in branches] + [np.zeros(0, np.uint8)])
            nv, total = I.crack_vertices(branches, points, keep, widths=wide)
            want, want_nv, want_total = SV.vertex_dicts(branches, tol_q)
            assert nv == want_nv and type(nv) is int and type(total) is float and abs(total - want_total) <= 1e-12 * max(want_total, 1.0)
            width = np.atleast_1d(I.width_from_d2(points[:, 3]))
            at = np.concatenate([np.zeros(1, np.int64), np.cumsum([len(b["points"]) for b in branches])]).tolist()
            for b, w, o0 in zip(branches, want, at):
                assert b["vertices"].dtype == np.int32 and np.array_equal(b["vertices"], w["vertices"]) and b["vertices"].shape == (len(w["vertex_index"]), 2)
                assert b["vertex_index"].dtype == np.int32 and np.array_equal(b["vertex_index"], w["vertex_index"])
                assert np.array_equal(b["points"][b["vertex_index"]], b["vertices"])
                if b["chain"]:
                    assert abs(b["length_simplified_px"] - w["length_simplified_px"]) <= 1e-12 * max(w["length_simplified_px"], 1.0)
                else:
                    assert b["length_simplified_px"] is None and b["vertices"].shape == (0, 2)
                assert ("vertex_width_px" in b) == wide
                if wide:
                    assert b["vertex_width_px"].dtype == np.float64 and b["vertex_width_px"].shape == b["vertex_index"].shape
                    assert np.array_equal(b["vertex_width_px"], width[o0 + b["vertex_index"]])
            totals.append(total)
        run, ring, dot, quad = rows[0][1]
        assert ring["length_simplified_px"] == I.polyline_length(ring["vertices"], closed=True) > I.polyline_length(ring["vertices"])
        assert dot["length_simplified_px"] == 0.0 and dot["vertices"].tolist() == [[0, 9]]
        if tol_q >= 2:
            assert run["vertices"].tolist() == [[7, 0], [7, 8], [9, 10]] and run["length_simplified_px"] == 8 + 2 * math.sqrt(2.0)
            assert rows[1][1][0]["vertices"].tolist() == [[1, 1], [3, 3]]
        # crack_vertices.csv
        path = str(tmp_path / f"crack_vertices_{tol_q}.csv")
        I.write_crack_vertices(path, rows)
        back = I.read_crack_vertices(path)
        assert [name for name, _ in back] == ["a.png", "b.png"]
        for (_, branches), (_, got) in zip(rows, back):
            kept = [(j, b) for j, b in enumerate(branches) if b["chain"]]
            assert [d["branch"] for d in got] == [j for j, _ in kept]
            for (j, b), d in zip(kept, got):
                assert d["vertices"].dtype == np.int32 and np.array_equal(d["vertices"], b["vertices"]) and np.array_equal(d["vertex_index"], b["vertex_index"])
                assert ("width_px" in d) == wide and (not wide or np.array_equal(d["width_px"], b["vertex_width_px"]))
        import skeleton_cases as SC
        assert SC.read_csv(path)[0] == I.VERTEX_CSV_COLUMNS + (I.VERTEX_CSV_OPTIONAL if wide else [])
        # crack_polylines.geojson
        gpath = str(tmp_path / f"crack_polylines_{tol_q}.geojson")
        I.write_crack_geojson(gpath, rows)
        text = open(gpath).read()
        doc = json.loads(text)
        assert text == json.dumps(doc, sort_keys=True) + "\n" and doc["type"] == "FeatureCollection"
        chains = [(name, j, b) for name, branches in rows for j, b in enumerate(branches) if b["chain"]]
        assert len(doc["features"]) == len(chains) == 4
        for f, (name, j, b) in zip(doc["features"], chains):
            p, g = f["properties"], f["geometry"]
            assert f["type"] == "Feature" and (p["name"], p["branch"], p["kind"], p["px"], p["crack"]) == (name, j, b["kind"], b["px"], b["crack"])
            assert p["n_vertices"] == len(b["vertices"]) and p["length_simplified_px"] == b["length_simplified_px"] and p["arc_px"] == b["arc_px"]
            assert p["closed"] is (b["kind"] == "ring") and ("max_width_px" in p) == wide and ("min_width_px" in p) == wide
            xy = [[x, y] for y, x in b["vertices"].tolist()]
            if len(xy) == 1:
                assert g == {"type": "Point", "coordinates": xy[0]}
            else:
                assert g == {"type": "LineString", "coordinates": xy + (xy[:1] if p["closed"] else [])}
    with open(path, "w") as fh:
        fh.write("name,branch,y,x\n")
    with pytest.raises(ValueError):
        I.read_crack_vertices(path)
    with pytest.raises(ValueError):
        I.crack_vertices(rows[1][1], np.zeros((3, 4), np.int32), np.zeros(2, np.uint8))
