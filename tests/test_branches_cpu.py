"""The NumPy restatement of the crack branches (tests/branch_cases.py) against a brute-force flood over the links, the kernel's tiles and
seams in Python, hand-written branch counts and kinds, the identities that tie the branch sums to the topology counts, the host helpers of
utils/estimate_metrics.py, the CSV writer and reader of inference.py and predict_dataset's argument checks.  Nothing here needs a GPU."""
import numpy as np
import pytest

import branch_cases as BC
import components_cases as CC
import skeleton_cases as SC
import topology_cases as TC

C = {k: j for j, k in enumerate(BC.COLUMNS)}


def _small_planes():
    """planes up to 12 x 12: every hand shape's corner, noise at five densities and three shapes, lines and blocks"""
    rng = np.random.default_rng(31)
    out = [BC.hand(k)[:9, :11] for k in BC.HAND]
    for shape in ((12, 12), (5, 7), (1, 12), (12, 1), (3, 3)):
        out += [(rng.random(shape) < d).astype(np.uint8) for d in (0.1, 0.3, 0.5, 0.7, 0.9)]
    return out + [np.ones((4, 6), np.uint8), np.zeros((3, 5), np.uint8), np.ones((1, 1), np.uint8)]


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_equals_a_flood_over_the_links():
    for plane in _small_planes():
        topo = TC.topo_of(plane)
        assert np.array_equal(BC.blabels_of(topo), BC.flood(topo))


def test_the_tiles_and_seams_give_the_same_labels_at_small_tiles():
    """4 x 8 tiles on planes up to 12 x 12: every seam kind occurs"""
    crossing = 0
    for plane in _small_planes():
        topo = TC.topo_of(plane)
        got, n = BC.kernel_form(topo, 4, 8)
        crossing += n
        assert np.array_equal(got, BC.blabels_of(topo))
    assert crossing > 20


@pytest.mark.parametrize("name", ["seams", "borders", "corner_strokes", "seam_T", "noise_0.05", "noise_0.3", "noise_0.6", "noise_0.95", "cracks",
                                  "cracks_pruned", "noise_130x260", "ones_65x129", "framed_batch", "two_and_one"])
def test_the_tiles_and_seams_give_the_same_labels(name):
    for topo, want in zip(*BC.expected(name)[:2]):
        assert np.array_equal(BC.kernel_form(topo)[0], want)


def test_the_corner_strokes_cross_every_seam_with_every_link_kind():
    """of the six (seam, kind) pairs the merge launch handles, the diagonal ones all occur: SE and SW over the row seam, SE out of a last
    column, SW out of a first column"""
    seen = set()
    for topo in BC.expected("corner_strokes")[0]:
        W = topo.shape[1]
        for p, q, k in BC.partition(topo)[0]:
            (py, px), (qy, qx) = divmod(p, W), divmod(q, W)
            if py // BC.TH != qy // BC.TH:
                seen.add(("row", k))
            if px // BC.TW != qx // BC.TW:
                seen.add(("column", k))
    assert {("row", 2), ("row", 3), ("column", 2), ("column", 3), ("row", 1), ("column", 0)} <= seen


def test_the_seam_T_has_its_junction_on_the_seam_and_its_arms_in_three_tiles():
    for topo, bl in zip(*BC.expected("seam_T")[:2]):
        (jy, jx), = np.argwhere(BC.is_junction(topo))
        assert jy in (63, 64) and jx in (127, 128)
        rows = BC.rows_of(topo[None])
        assert len(rows) == 3 and BC.kinds_of(rows) == ["terminal"] * 3 and (rows[:, C["attach"]] == 1).all()
        tiles = [{(y // BC.TH, x // BC.TW) for y, x in np.argwhere(bl == lab)} for lab in rows[:, 1]]
        assert all(len(t) == 1 for t in tiles) and len(set.union(*tiles)) == 3


# ------------------------------------------------------------------------------------------------ hand shapes
@pytest.mark.parametrize("name", list(BC.HAND))
def test_hand_shapes_have_their_hand_written_branches(name):
    _, n, kinds, junction_px = BC.HAND[name]
    topo = TC.topo_of(BC.hand(name))
    rows = BC.rows_of(topo[None])
    assert len(rows) == n and sorted(BC.kinds_of(rows)) == sorted(kinds) and int(BC.is_junction(topo).sum()) == junction_px


def test_the_arms_of_a_T_get_three_labels_where_8_connectivity_gives_one():
    plane = BC.hand("T")
    topo = TC.topo_of(plane)
    bl = BC.blabels_of(topo)
    assert len(set(bl[bl != 0].tolist())) == 3 and bl[2, 5] == 0                     # the junction pixel carries no label
    assert len(set(CC.canonical_labels(BC.is_branch(topo), 8).ravel().tolist()) - {0}) == 1      # (2, 4) and (3, 5) touch diagonally
    rows = BC.rows_of(topo[None])
    assert sorted(rows[:, C["px"]].tolist()) == [2, 2, 2] and (rows[:, C["node_a"]] == rows[:, C["node_b"]]).all()
    # a length runs to the centre of the junction pixel: two arms of 2 links along the bar, the stem of 2 links down
    assert sorted(zip(rows[:, C["h"]].tolist(), rows[:, C["v"]].tolist())) == [(0, 2), (2, 0), (2, 0)]


def test_a_ring_without_a_junction_is_one_ring_branch():
    for name in ("ring", "diamond"):
        rows = BC.rows_of(TC.topo_of(BC.hand(name))[None])
        r = dict(zip(BC.COLUMNS, rows[0].tolist()))
        assert len(rows) == 1 and BC.kinds_of(rows) == ["ring"] and (r["end"], r["attach"], r["node_a"], r["node_b"]) == (0, 0, 0, 0)
        assert r["px"] == len(BC.HAND[name][0]) == r["h"] + r["v"] + r["d_se"] + r["d_sw"]


def test_the_figure_eight_is_two_self_loops_on_one_junction():
    topo = TC.topo_of(BC.hand("eight"))
    rows = BC.rows_of(topo[None])
    assert (rows[:, C["attach"]] == 2).all() and (rows[:, C["node_a"]] == rows[:, C["node_b"]]).all() and (rows[:, C["node_a"]] > 0).all()
    assert (rows[:, C["d_se"]] + rows[:, C["d_sw"]] == 8).all() and (rows[:, C["px"]] == 7).all()


# ------------------------------------------------------------------------------------------------ identities
IDENTITY_CASES = ["seams", "borders", "corner_strokes", "seam_T", "noise_0.05", "noise_0.3", "noise_0.6", "noise_0.95", "cracks", "cracks_pruned",
                  "framed_batch", "two_and_one", "ones", "zeros", "noise_5x7", "ones_1x1"]


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_the_sums_tie_to_the_topology_counts(name):
    topo_all, bl_all, _ = BC.expected(name)
    for topo, bl in zip(topo_all, bl_all):
        counts = dict(zip(TC.COLUMNS, (int(k) for k in TC.counts_of(topo))))
        inner, attach, cluster = (len(p) for p in BC.partition(topo))
        assert inner + attach + cluster == counts["h"] + counts["v"] + counts["d_se"] + counts["d_sw"]
        rows = BC.rows_of(topo[None])
        assert rows[:, C["end"]].sum() == counts["end"] and rows[:, C["isolated"]].sum() == counts["isolated"]
        assert rows[:, C["px"]].sum() == counts["V"] - counts["junction_px"]
        assert rows[:, C["attach"]].sum() == attach and rows[:, [C["h"], C["v"], C["d_se"], C["d_sw"]]].sum() == inner + attach
        assert BC.kinds_of(rows).count("isolated") == counts["isolated"]
        assert (rows[:, 1] == np.unique(bl[bl != 0])).all()


@pytest.mark.parametrize("seed", TC.CRACK_SEEDS)
def test_the_crack_skeletons_have_their_branches(seed):
    topo = TC.topo_of(TC.crack_skeleton(seed))
    assert len(BC.rows_of(topo[None])) == BC.BRANCH_COUNTS[seed]
    assert tuple(len(p) for p in BC.partition(topo)) == BC.PARTITIONS[seed]
    assert TC.junctions_of(TC.crack_skeleton(seed)) == {0: 45, 1: 43, 2: 50}[seed]
    assert SC.components(BC.is_branch(topo)) == {0: 37, 1: 37, 2: 54}[seed]          # what 8-connectivity of the non-junction pixels leaves joined


@pytest.mark.parametrize("name", ["cracks", "noise_0.3", "corner_strokes", "two_and_one"])
def test_the_branches_of_a_plane_are_the_union_of_the_branches_of_its_components(name):
    for plane in BC.cases()[name]:
        lab = CC.canonical_labels(plane != 0, 8)
        whole = BC.rows_of(TC.topo_of(plane)[None], labels=lab[None])
        parts = [BC.rows_of(TC.topo_of(plane * (lab == k))[None], labels=lab[None]) for k in np.unique(lab[lab != 0])]
        parts = np.concatenate(parts) if parts else whole[:0]
        # a component's junction clusters keep their first pixels, so the node columns agree too
        assert np.array_equal(whole, parts[np.argsort(parts[:, 1], kind="stable")])
        assert (whole[:, C["crack"]] > 0).all()


def test_a_branch_may_touch_more_than_two_clusters():
    """the documented bias: one branch of seed 0 and one of seed 2 attach to junction pixels of three or more clusters, none of seed 1; such
    a branch names only the smallest and the largest cluster and its attach exceeds 2"""
    many = {}
    for seed in TC.CRACK_SEEDS:
        topo = TC.topo_of(TC.crack_skeleton(seed))
        bl, jl = BC.blabels_of(topo).ravel(), BC.junction_labels(topo).ravel()
        clusters = {}
        for p, q, _ in BC.partition(topo)[1]:
            b, j = (p, q) if bl[p] else (q, p)
            clusters.setdefault(int(bl[b]), set()).add(int(jl[j]))
        many[seed] = sorted(len(c) for c in clusters.values() if len(c) > 2)
        rows = BC.rows_of(topo[None])
        for r in rows[np.isin(rows[:, 1], [k for k, c in clusters.items() if len(c) > 2])]:
            assert r[C["attach"]] > 2 and r[C["node_a"]] == min(clusters[int(r[1])]) and r[C["node_b"]] == max(clusters[int(r[1])])
    assert many == {0: [4], 1: [], 2: [3]}


def test_the_sums_with_a_width_map():
    topo, bl, jl = BC.expected("cracks")
    d2 = BC.fake_d2(bl)
    rows = BC.rows_of(topo, d2=d2)
    assert rows.shape[1] == 19 and np.array_equal(rows[:, :17], BC.rows_of(topo))
    for r in rows[::7]:
        v = d2[r[0]][bl[r[0]] == r[1]]
        assert r[17] == v.max() and r[18] == (v[v > 0].min() if (v > 0).any() else 0)
    assert (rows[:, 18] == 0).any() or (rows[:, 18] <= rows[:, 17]).all()


# ------------------------------------------------------------------------------------------------ the host helpers
KIND_TABLE = [  # end, attach, node_a, node_b, isolated -> kind
    ((0, 0, 0, 0, 1), "isolated"), ((2, 0, 0, 0, 0), "free"), ((0, 0, 0, 0, 0), "ring"), ((1, 1, 7, 7, 0), "terminal"), ((1, 2, 3, 9, 0), "terminal"),
    ((2, 1, 3, 3, 0), "terminal"), ((0, 2, 5, 5, 0), "self_loop"), ((0, 1, 5, 5, 0), "self_loop"), ((0, 2, 5, 8, 0), "link"), ((0, 4, 2, 90, 0), "link"),
    ((1, 0, 0, 0, 0), "link"), ((3, 0, 0, 0, 0), "link"),
]


@pytest.mark.parametrize("args,kind", KIND_TABLE)
def test_branch_kind_matches_its_truth_table(args, kind):
    from csbsr_amd.utils import estimate_metrics as M
    assert M.branch_kind(*args) == kind == BC.kind_of(*args) and kind in M.BRANCH_KINDS
    assert M.branch_kind(*(np.int32(a) for a in args)) == kind


def test_the_names_agree_with_the_restatement():
    from csbsr_amd.utils import estimate_metrics as M
    assert M.BRANCH_COLUMNS == BC.COLUMNS and M.BRANCH_WIDTH_COLUMNS == BC.WIDTH_COLUMNS and M.BRANCH_KINDS == BC.KINDS and M.BRANCH_ACC == 12


def _row(**kw):
    return [kw.get(k, 0) for k in BC.COLUMNS]


def test_summarize_branches_on_hand_made_rows():
    from csbsr_amd.utils import estimate_metrics as M
    rows = np.array([_row(label=1, px=1, isolated=1),
                     _row(label=9, px=5, end=2, h=4),                                               # free, length 4
                     _row(label=20, px=8, d_se=4, d_sw=4),                                          # ring, length 8 sqrt 2
                     _row(label=31, px=3, end=1, attach=1, v=3, node_a=4, node_b=4),                # terminal, length 3
                     _row(label=40, px=2, attach=2, h=3, node_a=4, node_b=6),                       # link, length 3
                     _row(label=50, px=6, attach=2, h=3, v=2, d_se=2, node_a=6, node_b=6)], np.int32)            # self_loop
    s = M.summarize_branches(rows)
    assert s["n_branches"] == 6 and s["branch_kinds"] == dict(isolated=1, free=1, ring=1, terminal=1, self_loop=1, link=1)
    assert list(s["branch_kinds"]) == list(M.BRANCH_KINDS)
    lengths = sorted([4.0, 8 * TC.SQRT2, 3.0, 3.0, 5 + 2 * TC.SQRT2])
    assert s["longest_branch_px"] == 8 * TC.SQRT2 and s["median_branch_px"] == lengths[2] == 4.0 and s["total_branch_px"] == float(np.sum(lengths))
    assert all(type(s[k]) is float for k in ("longest_branch_px", "median_branch_px", "total_branch_px"))
    assert M.branch_kinds(rows) == ["isolated", "free", "ring", "terminal", "link", "self_loop"]
    wide = np.concatenate([rows, np.ones((6, 2), np.int32)], 1)                       # with the width columns: the same figures
    assert M.summarize_branches(wide) == s
    only_isolated = M.summarize_branches(rows[:1])
    assert only_isolated["n_branches"] == 1 and only_isolated["longest_branch_px"] == only_isolated["median_branch_px"] == 0.0
    empty = M.summarize_branches(np.zeros((0, 17), np.int32))
    assert empty == dict(n_branches=0, branch_kinds={k: 0 for k in M.BRANCH_KINDS}, longest_branch_px=0.0, median_branch_px=0.0, total_branch_px=0.0)
    for bad in (np.zeros((3, 16), np.int32), np.zeros(17, np.int32), np.zeros((2, 18), np.int32)):
        with pytest.raises(ValueError):
            M.summarize_branches(bad)


def test_summarize_branches_on_the_crack_skeletons():
    from csbsr_amd.utils import estimate_metrics as M
    for seed in TC.CRACK_SEEDS:
        rows = BC.rows_of(TC.topo_of(TC.crack_skeleton(seed))[None])
        s = M.summarize_branches(rows)
        kinds = BC.kinds_of(rows)
        assert s["n_branches"] == BC.BRANCH_COUNTS[seed] and s["branch_kinds"] == {k: kinds.count(k) for k in BC.KINDS}
        lengths = sorted(TC.length(*r[[C["h"], C["v"], C["d_se"], C["d_sw"]]].tolist()) for r in rows if not r[C["isolated"]])
        assert s["longest_branch_px"] == lengths[-1] and s["median_branch_px"] == lengths[(len(lengths) - 1) // 2]


def test_crack_branches_builds_the_dicts_of_the_restatement():
    from csbsr_amd import inference as I
    topo, bl, _ = BC.expected("cracks")
    W = topo.shape[2]
    lab = CC.canonical_labels(topo[0] != 0, 8)
    rows = BC.rows_of(topo[:1], labels=lab[None], d2=BC.fake_d2(bl[:1]))
    of_label = {int(k): j for j, k in enumerate(np.unique(lab[lab != 0]))}
    got, want = I.crack_branches(rows, W, of_label), BC.branch_dicts(rows, W, of_label)
    assert got == want and len(got) == BC.BRANCH_COUNTS[0]
    assert set(got[0]) == {"y", "x", "kind", "px", "ends", "attach", "nodes", "links", "length_geodesic_px", "orientation", "bbox", "crack",
                           "max_width_px", "min_width_px"}
    assert all(type(b["length_geodesic_px"]) is float and type(b["links"]) is tuple and type(b["px"]) is int for b in got)
    plain = I.crack_branches(rows[:, :17], W)
    assert plain == BC.branch_dicts(rows[:, :17], W) and "crack" not in plain[0] and "max_width_px" not in plain[0]


def test_the_csv_file_round_trips(tmp_path):
    from csbsr_amd import inference as I
    topo, bl, _ = BC.expected("cracks")
    W = topo.shape[2]
    lab = CC.canonical_labels(topo[1] != 0, 8)
    of_label = {int(k): j for j, k in enumerate(np.unique(lab[lab != 0]))}
    wide = BC.rows_of(topo[1:2], labels=lab[None], d2=BC.fake_d2(bl[1:2]))
    for tag, a, b in (("plain", I.crack_branches(BC.rows_of(topo[:1]), W), I.crack_branches(BC.rows_of(topo[2:]), W)),
                      ("crack", I.crack_branches(wide[:, :17], W, of_label), I.crack_branches(wide[:5, :17], W, of_label)),
                      ("width", I.crack_branches(wide[:, :], W), []),
                      ("both", I.crack_branches(wide, W, of_label), I.crack_branches(wide[3:9], W, of_label))):
        path = str(tmp_path / f"{tag}.csv")
        rows = [("a.png", a), ("b.png", b)]
        I.write_crack_branches(path, rows)
        assert I.read_crack_branches(path) == [(n, r) for n, r in rows if r]
        with open(path) as fh:
            header = fh.readline().strip().split(",")
        assert header[:len(I.BRANCH_CSV_COLUMNS)] == I.BRANCH_CSV_COLUMNS
        assert header[len(I.BRANCH_CSV_COLUMNS):] == [k for k in I.BRANCH_CSV_OPTIONAL if k in a[0]]
    path = str(tmp_path / "none.csv")
    I.write_crack_branches(path, [("a.png", []), ("b.png", [])])                     # no branch at all: the header alone
    assert I.read_crack_branches(path) == []
    with open(path, "w") as fh:
        fh.write("name,crack\n")
    with pytest.raises(ValueError):
        I.read_crack_branches(path)


# ------------------------------------------------------------------------------------------------ refusals
def test_predict_dataset_refuses_a_bad_branches_argument_before_the_model_runs():
    from csbsr_amd.inference import predict_dataset
    model = lambda *a, **kw: pytest.fail("the model ran")
    t = 0.4
    for kwargs in (dict(branches=True), dict(measure_threshold=t, branches=True), dict(measure_threshold=t, topology=False, branches=True),
                   dict(measure_threshold=t, min_crack_px=5, branches=True), dict(topology=True, branches=True),
                   dict(measure_threshold=t, topology=True, branches=1), dict(measure_threshold=t, topology=True, branches=None),
                   dict(measure_threshold=t, topology=True, branches="True"), dict(measure_threshold=t, topology=True, branches=0)):
        with pytest.raises(ValueError):
            next(predict_dataset(model, None, **kwargs))


def test_the_table_builders_refuse_what_is_no_device_tensor():
    import torch
    from csbsr_amd.utils import estimate_metrics as M
    for bad in (np.zeros((1, 4, 4), np.uint8), torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            M.label_branches(bad)
    for bad in (np.zeros((1, 4, 4), np.int32), torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(1, 4, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError):                                              # a host tensor is no blabels of label_branches
            M.branch_table(bad, torch.zeros(1, 4, 4, dtype=torch.uint8))
