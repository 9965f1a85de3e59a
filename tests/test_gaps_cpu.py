"""The NumPy restatement of the crack gap bridging (tests/gap_cases.py) against itself and against values written out by hand, and the host
side of csbsr_amd: gap_radius, summarize_gaps, the crack_gaps.csv writer / reader, the ABI table and predict_dataset's argument checks.
Nothing here needs a GPU; tests/test_gaps_gpu.py holds the device equal to this restatement."""
import inspect
import os
import re

import numpy as np
import pytest

import gap_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gaps(name, G, to="any"):
    """{(py, px): ((qy, qx), d2)} of a one-plane case"""
    gq, gd = GC.expected(name, G, to)[:2]
    W = gq.shape[2]
    return {(int(y), int(x)): (divmod(int(gq[0, y, x]), W), int(gd[0, y, x])) for y, x in zip(*np.nonzero(gq[0] >= 0))}


# ------------------------------------------------------------------------------------------------ the two forms
@pytest.mark.parametrize("name", list(GC.cases()))
def test_the_two_forms_of_the_search_agree(name):
    topo, labels = GC.cases()[name]
    for G in GC.gaps_for(name):
        for to in GC.TOS:
            gq, gd = GC.expected(name, G, to)[:2]
            wq, wd = GC.gaps_window(topo, labels, G, to)
            assert np.array_equal(gq, wq) and np.array_equal(gd, wd), (G, to)
            cls = topo & 7
            src = ((cls == 1) | (cls == 2)) & (labels != 0)
            assert not (gq[~src] != -1).any() and not gd[gq < 0].any() and (gd[gq >= 0] >= 4).all() and (gd <= G * G).all()


def test_the_pinned_counts_of_the_crack_cases():
    for mask in GC.CRACK_MASKS:
        topo, labels = GC.crack_case(mask)
        got = tuple(int((GC.gaps_brute(topo, labels, G)[0] >= 0).sum()) for G in GC.CRACK_GAPS)
        assert got == GC.CRACK_COUNTS[mask], mask
    assert GC.CRACK_COUNTS == {(2, 67, 263): (9, 32, 52, 64), (6, 131, 135): (13, 46, 71, 86), (4, 70, 133): (7, 27, 46, 53)}


# ------------------------------------------------------------------------------------------------ hand values
def test_two_collinear_runs():
    assert _gaps("collinear", 4) == {(4, 8): ((4, 12), 16), (4, 12): ((4, 8), 16)} == _gaps("collinear", 4, "end")
    gq, gd, table, groups, bridges = GC.expected("collinear", 4, "any")
    W = gq.shape[2]
    first, second = 4 * W + 2 + 1, 4 * W + 12 + 1
    assert table.tolist() == [[0, 4 * W + 8, 4 * W + 12, 16, first, second, 2, 1], [0, 4 * W + 12, 4 * W + 8, 16, second, first, 2, 1]]
    assert set(np.unique(groups)) == {0, first} and (groups[0, 4, 12:19] == first).all()              # one group
    assert [tuple(v) for v in np.argwhere(bridges[0])] == [(4, x) for x in range(8, 13)]
    sk = (GC.cases()["collinear"][0][0] & 7) != 0
    assert [tuple(v) for v in np.argwhere((bridges[0] != 0) & ~sk)] == [(4, 9), (4, 10), (4, 11)]     # bridge_px 3
    assert _gaps("collinear", 3) == {} and not GC.expected("collinear", 3, "any")[4].any()
    assert np.array_equal(GC.expected("collinear", 3, "any")[3], GC.cases()["collinear"][1])


def test_a_tee_that_does_not_touch():
    for G in (3, 4, 7):
        assert _gaps("tee", G) == {(7, 11): ((10, 11), 9)}
    row = GC.expected("tee", 4, "any")[2]
    assert row.shape == (1, 8) and row[0, 6] == 3 and row[0, 7] == 0                                  # an end_side gap; the path pixel has none
    # "end": (10, 2) and (10, 20) are both 90 away from (7, 11); the smaller index wins
    assert _gaps("tee", 10, "end") == {(7, 11): ((10, 2), 90), (10, 2): ((7, 11), 90), (10, 20): ((7, 11), 90)}
    assert GC.expected("tee", 10, "end")[2][:, 7].tolist() == [1, 1, 0]
    assert _gaps("tee", 9, "end") == {}


def test_a_u_has_no_gap_to_itself():
    topo = GC.cases()["u_shape"][0]
    assert sorted(tuple(v) for v in np.argwhere((topo[0] & 7) == 2)) == [(2, 3), (2, 6)]
    for G in GC.GAPS:
        assert _gaps("u_shape", G) == {} == _gaps("u_shape", G, "end")


def test_an_isolated_pixel_is_a_source_and_a_target():
    assert (GC.cases()["isolated_beside"][0][0, 5, 5] & 7) == 1
    assert _gaps("isolated_beside", 2) == {(5, 5): ((3, 5), 4)} and _gaps("isolated_beside", 2, "end") == {}
    want = {(5, 5): ((3, 5), 4), (3, 2): ((5, 5), 13), (3, 8): ((5, 5), 13)}
    assert _gaps("isolated_beside", 5) == want
    assert _gaps("isolated_beside", 5, "end") == {**want, (5, 5): ((3, 2), 13)}                 # (3, 2) before (3, 8)
    assert GC.expected("isolated_beside", 5, "any")[2][:, 6].tolist() == [1, 1, 3]                     # class_q: isolated, isolated, path


def test_a_pixel_without_a_label_is_neither_source_nor_target():
    topo, labels = GC.cases()["unlabelled_between"]
    assert (topo[0, 4, 9] & 7) == 2 and labels[0, 4, 9] == 0
    assert _gaps("unlabelled_between", 5) == {}                                                       # (4, 6) and (4, 9) are 3 apart
    assert _gaps("unlabelled_between", 10) == {(4, 6): ((4, 16), 100), (4, 16): ((4, 6), 100)}
    bridges = GC.expected("unlabelled_between", 10, "any")[4]
    assert [tuple(v) for v in np.argwhere(bridges[0])] == [(4, x) for x in range(6, 17)]               # over the unlabelled run
    assert not GC.expected("unlabelled_between", 10, "any")[3][0, 4, 9:14].any()                       # which stays in no group


def test_no_gap_leads_into_another_plane():
    topo = GC.cases()["two_planes"][0]
    assert (topo[0, 7, 5] & 7) == 2 and (topo[1, 0, 5] & 7) == 2
    for G in GC.GAPS:
        for to in GC.TOS:
            assert not (GC.expected("two_planes", G, to)[0] >= 0).any()


def test_ends_at_corners_and_borders():
    got = _gaps("borders", 3)
    assert got[(0, 0)] == ((3, 0), 9) and got[(3, 0)] == ((0, 0), 9) and (0, 20) not in got
    got = _gaps("borders", 64)
    topo = GC.cases()["borders"][0]
    assert set(got) == {tuple(v) for v in np.argwhere(np.isin(topo[0] & 7, (1, 2)))}                  # everything is within 64 of something
    assert got[(0, 0)] == ((3, 0), 9) and got[(15, 20)] == ((12, 20), 9) and got[(0, 20)] == ((4, 20), 16) and got[(15, 0)] == ((10, 0), 25)


def test_equal_distances_go_to_the_first_in_raster_order():
    assert _gaps("equal_d2", 5)[(5, 5)] == ((2, 9), 25) and _gaps("equal_d2", 5, "end")[(5, 5)] == ((2, 9), 25)
    assert _gaps("equal_d2_second", 5)[(5, 5)] == ((5, 0), 25)
    assert _gaps("equal_d2", 5)[(0, 11)] == ((2, 9), 8) and (0, 11) not in _gaps("equal_d2_second", 5)
    assert (5, 5) not in _gaps("equal_d2", 4) and (5, 5) not in _gaps("equal_d2_second", 4)


def test_every_branch_of_the_bresenham_loop():
    assert GC.bresenham((2, 2), (4, 9)) == [(2, 2), (2, 3), (3, 4), (3, 5), (3, 6), (3, 7), (4, 8), (4, 9)]
    assert GC.bresenham((4, 25), (2, 32)) == [(2, 32), (2, 31), (3, 30), (3, 29), (3, 28), (3, 27), (4, 26), (4, 25)]
    assert GC.bresenham((14, 2), (21, 4)) == [(14, 2), (15, 2), (16, 3), (17, 3), (18, 3), (19, 3), (20, 4), (21, 4)]
    assert GC.bresenham((14, 30), (21, 28)) == [(14, 30), (15, 30), (16, 29), (17, 29), (18, 29), (19, 29), (20, 28), (21, 28)]
    assert GC.bresenham((30, 2), (35, 7)) == [(30 + i, 2 + i) for i in range(6)]
    assert GC.bresenham((35, 27), (30, 32)) == [(30 + i, 32 - i) for i in range(6)]
    assert GC.bresenham((44, 8), (44, 2)) == [(44, x) for x in range(2, 9)] and GC.bresenham((3, 3), (3, 3)) == [(3, 3)]
    assert GC.bresenham((50, 25), (44, 25)) == [(y, 25) for y in range(44, 51)]
    got = _gaps("bridge_pairs", 8)
    for a, b in GC.BRIDGE_PAIRS:
        d2 = (a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2
        assert got[a] == (b, d2) and got[b] == (a, d2)
    want = np.zeros((56, 36), np.uint8)
    for a, b in GC.BRIDGE_PAIRS:
        line = GC.bresenham(a, b)
        assert line == GC.bresenham(b, a) and len(line) == max(abs(a[0] - b[0]), abs(a[1] - b[1])) + 1           # the smaller index draws
        assert all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) == 1 for p, q in zip(line, line[1:]))                 # 8-connected
        for y, x in line:
            want[y, x] = 1
    assert np.array_equal(GC.expected("bridge_pairs", 8, "any")[4][0], want)


def test_the_tile_cases():
    got = _gaps("tile_seams", 5)
    assert got[(62, 20)] == ((66, 20), 16) and got[(66, 20)] == ((62, 20), 16)                         # the horizontal seam
    assert got[(10, 126)] == ((10, 129), 9) and got[(10, 129)] == ((10, 126), 9)                       # the vertical seam
    assert got[(62, 126)] == ((65, 129), 18) and got[(65, 129)] == ((62, 126), 18)                     # the corner of the four tiles
    assert got[(34, 129)] == ((34, 132), 9) and got[(32, 132)] == ((32, 129), 9)                       # the last word's remainder: end to side
    got = _gaps("across_a_tile", 64)
    assert got == {(63, 250): ((127, 250), 4096), (127, 250): ((63, 250), 4096), (5, 100): ((5, 164), 4096), (5, 164): ((5, 100), 4096)}
    assert _gaps("across_a_tile", 16) == {}


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("name", list(GC.cases()))
def test_tables_groups_and_bridges(name):
    topo, labels = GC.cases()[name]
    N, H, W = labels.shape
    for G in GC.gaps_for(name):
        for to in GC.TOS:
            gq, gd, table, groups, bridges = GC.expected(name, G, to)
            assert table.dtype == np.int32 and table.shape == (int((gq >= 0).sum()), 8)
            # mutual gaps are symmetric: the row of q names p, with the same d2
            rows = {(n, p): (q, d2, m) for n, p, q, d2, _, _, _, m in table.tolist()}
            for (n, p), (q, d2, m) in rows.items():
                assert bool(m) == (rows.get((n, q), (None,))[0] == p) and (not m or rows[(n, q)][1] == d2)
            assert (table[:, 4] != table[:, 5]).all() and (table[:, 4] > 0).all() and (table[:, 5] > 0).all()
            assert (table[:, 6] >= (1 if to == "any" else 1)).all() and (to == "any" or np.isin(table[:, 6], (1, 2)).all())
            # the group label is the smallest label of the group, and both forms of the grouping agree
            assert np.array_equal(groups, GC.groups_union_find(labels, gq))
            assert ((groups == 0) == (labels == 0)).all() and (groups <= labels).all()
            for n in range(N):
                for g in np.unique(groups[n])[1:]:
                    assert labels[n][groups[n] == g].min() == g
                fl, fg = labels[n].ravel(), groups[n].ravel()
                p = np.nonzero(gq[n].ravel() >= 0)[0]
                assert np.array_equal(fg[p], fg[gq[n].ravel()[p]])                                     # a gap's two ends are in one group
            assert np.array_equal(GC.groups_of(groups, gq), groups)                                    # grouping twice changes nothing
            # bridges: both ends plotted, nothing without a gap
            assert bridges.dtype == np.uint8 and bridges.max(initial=0) <= 1 and bool(bridges.any()) == bool(len(table))
            n, y, x = np.nonzero(gq >= 0)
            assert bridges[n, y, x].all() and bridges.reshape(N, -1)[n, gq[n, y, x]].all()


def test_summarize_gaps():
    from csbsr_amd.utils import estimate_metrics as M
    assert M.GAP_MAX_RADIUS == GC.MAX_G == 64 and M.GAP_COLUMNS == GC.COLUMNS
    none = M.summarize_gaps(np.zeros((0, 8), np.int32), 3)
    assert none == dict(n_gaps=0, n_mutual=0, n_end_to_end=0, n_end_to_side=0, gap_length_px=0.0, max_gap_px=0.0, n_cracks_bridged=3)
    assert M.summarize_gaps([], 0)["n_cracks_bridged"] == 0
    table = GC.expected("collinear", 4, "any")[2]
    got = M.summarize_gaps(table, 2)                                                                   # a mutual pair counted once
    assert got == dict(n_gaps=2, n_mutual=2, n_end_to_end=2, n_end_to_side=0, gap_length_px=4.0, max_gap_px=4.0, n_cracks_bridged=1)
    got = M.summarize_gaps(GC.expected("tee", 10, "end")[2], 2)
    assert got["n_gaps"] == 3 and got["n_mutual"] == 2 and got["gap_length_px"] == 2 * 90 ** 0.5 and got["n_cracks_bridged"] == 1
    for name in GC.cases():
        topo, labels = GC.cases()[name]
        for G in GC.gaps_for(name)[-2:]:
            table = GC.expected(name, G, "any")[2]
            for n in range(labels.shape[0]):
                rows = table[table[:, 0] == n]
                k = len(np.unique(labels[n])) - 1
                got, want = M.summarize_gaps(rows, k), GC.summary_of(rows, k)
                assert set(got) == set(want) and all(type(got[q]) is type(want[q]) for q in got)
                assert abs(got.pop("gap_length_px") - want.pop("gap_length_px")) <= 1e-12 * max(1.0, want["max_gap_px"] * len(rows)) and got == want
                assert got["n_cracks_bridged"] == len(np.unique(GC.expected(name, G, "any")[3][n])) - 1
                assert M.gap_group_of(rows) == {int(a): int(b) for a, b in zip(labels[n].ravel(), GC.expected(name, G, "any")[3][n].ravel())
                                                if a in set(rows[:, 4:6].ravel().tolist())}
    assert M.gap_length(16) == 4.0 and type(M.gap_length(16)) is float and M.gap_length(np.array([0, 2, 9])).tolist() == [0.0, 2 ** 0.5, 3.0]
    for bad in ((np.zeros((2, 7)), 1), (np.zeros((0, 8)), -1), (np.zeros((0, 8)), True), (np.zeros((0, 8)), 1.0)):
        with pytest.raises(ValueError):
            M.summarize_gaps(*bad)


def test_gap_radius_and_target():
    from csbsr_amd.utils import estimate_metrics as M
    assert [M.gap_radius(g) for g in (2, 64, np.int32(5), np.int64(16))] == [2, 64, 5, 16] and type(M.gap_radius(np.int32(5))) is int
    for bad in (1, 0, -2, 65, True, False, 2.0, np.float32(4), "4", None, [4], np.bool_(True)):
        with pytest.raises(ValueError, match="2 .. 64"):
            M.gap_radius(bad)
    assert M.gap_target("any") == "any" and M.gap_target("end") == "end"
    for bad in ("END", "", None, 1, True, ("end",)):
        with pytest.raises(ValueError):
            M.gap_target(bad)


def test_the_device_entries_refuse_what_is_no_device_tensor():
    import torch
    from csbsr_amd.utils import estimate_metrics as M
    topo, labels = torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.int32)
    for call in (lambda: M.endpoint_gaps(topo, labels, 1), lambda: M.endpoint_gaps(topo, labels, 4, "side"), lambda: M.endpoint_gaps(topo, labels, 4),
                 lambda: M.endpoint_gaps(topo.numpy(), labels, 4), lambda: M.gap_groups(labels, labels), lambda: M.draw_bridges(labels),
                 lambda: M.draw_bridges(labels.numpy()), lambda: M.gap_table(topo, labels, labels, labels)):
        with pytest.raises(ValueError):
            call()


def test_abi_matches_the_header():
    from csbsr_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    ctype = {"const uint8_t*": L.vp, "const int32_t*": L.vp, "uint8_t*": L.vp, "int32_t*": L.vp, "csbsr_stream_t": L.vp, "int32_t": L.i32}
    want = {"csbsr_gap_max_radius": ("int32_t", 0), "csbsr_endpoint_gaps": ("int", 10), "csbsr_gap_groups": ("int", 8), "csbsr_gap_draw": ("int", 6)}
    for name, (res, nargs) in want.items():
        decl = re.search(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert decl and decl.group(1) == res, f"{name} is not declared in include/csbsr_hip.h"
        text = decl.group(2).replace("\n", " ").strip()
        args = [] if text == "void" else [ctype[" ".join(a.split()[:-1])] for a in text.split(",")]
        r, sig = L.SIGNATURES[name]
        assert r is L.i32 and sig == args and len(args) == nargs
    assert "gaps.hip" in open(os.path.join(ROOT, "csbsr_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "csbsr_amd", "csrc", "gaps.hip")).read()
    defs = {k: int(re.search(r"#define\s+%s\s+(\d+)" % k, src).group(1)) for k in ("GP_TH", "GP_TWW", "GP_MAX_G", "GP_MAX_SIDE")}
    assert (defs["GP_TH"], 32 * defs["GP_TWW"], defs["GP_MAX_G"], defs["GP_MAX_SIDE"]) == (GC.TH, GC.TW, GC.MAX_G, 8192)
    assert int(re.search(r"#define\s+GP_WAVE_SRC\s+(\d+)", src).group(1)) == GC.WAVE_SRC                   # the grid cases sit on both sides of it
    for n in (GC.WAVE_SRC, GC.WAVE_SRC + 1):
        topo = GC.cases()[f"grid_{n}"][0]
        assert int(((topo[0, :GC.TH, :GC.TW] & 7) == 1).sum()) == n == int((topo != 0).sum())
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(float|double|asm)\b", code) and '#include "union_find.h"' in code and "cc_union<CC_AGENT>" in code


def test_predict_dataset_takes_bridge_gap_px_and_refuses_it_before_the_model_runs():
    from csbsr_amd.inference import predict_dataset
    par = inspect.signature(predict_dataset).parameters
    assert par["bridge_gap_px"].default is None and par["bridge_to"].default == "any"
    model = lambda *a, **kw: pytest.fail("the model ran")
    base = dict(measure_threshold=0.4, topology=True)
    for kwargs in (dict(bridge_gap_px=4), dict(bridge_gap_px=4, measure_threshold=0.4), dict(bridge_gap_px=4, topology=False, measure_threshold=0.4),
                   dict(bridge_gap_px=1, **base), dict(bridge_gap_px=65, **base), dict(bridge_gap_px=True, **base), dict(bridge_gap_px=4.0, **base),
                   dict(bridge_gap_px="4", **base), dict(bridge_gap_px=4, bridge_to="side", **base), dict(bridge_gap_px=4, bridge_to=None, **base),
                   dict(bridge_to="end"), dict(bridge_to="end", **base), dict(bridge_to="nearest"), dict(bridge_gap_px=0, **base)):
        with pytest.raises(ValueError):
            next(predict_dataset(model, None, **kwargs))


# ------------------------------------------------------------------------------------------------ the file
def test_crack_gaps_csv_round_trip(tmp_path):
    from csbsr_amd import inference as I
    import skeleton_cases as SC
    topo, labels = GC.cases()["tile_seams"]
    W = labels.shape[2]
    rows = GC.expected("tile_seams", 16, "any")[2]
    of_label = {int(v): k for k, v in enumerate(np.unique(labels)[1:])}
    for wide in (False, True):
        gaps = I.crack_gaps(rows, W, of_label if wide else None)
        want = GC.gap_dicts(rows, W, of_label if wide else None)
        assert gaps == want and len(gaps) > 8 and all(type(g["gap_px"]) is float and type(g["mutual"]) is bool and type(g["d2"]) is int for g in gaps)
        assert {g["kind"] for g in gaps} == {"end_end", "end_side"} and {g["mutual"] for g in gaps} == {True, False}
        data = [("a.png", gaps), ("none.png", []), ("b.png", gaps[3:5])]
        path = str(tmp_path / f"crack_gaps_{wide}.csv")
        I.write_crack_gaps(path, data)
        assert I.read_crack_gaps(path) == [d for d in data if d[1]]                                    # exactly: repr() of the fp64 length
        assert SC.read_csv(path)[0] == I.GAP_CSV_COLUMNS + (I.GAP_CSV_OPTIONAL if wide else [])
    I.write_crack_gaps(str(tmp_path / "empty.csv"), [("a.png", [])])
    assert I.read_crack_gaps(str(tmp_path / "empty.csv")) == []
    assert I.crack_gaps(np.zeros((0, 8), np.int32), W) == []
    with open(tmp_path / "bad.csv", "w") as fh:
        fh.write("name,gap\n")
    with pytest.raises(ValueError):
        I.read_crack_gaps(str(tmp_path / "bad.csv"))
