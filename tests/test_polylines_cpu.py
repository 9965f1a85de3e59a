"""The NumPy restatement of the crack polylines (tests/polyline_cases.py): the walk against the pointer-jumping form on every case, hand
values, where a branch is no chain and how much of a crack skeleton that leaves unordered, the host helpers of utils/estimate_metrics.py,
the CSV writer and reader of inference.py and predict_dataset's argument checks.  Nothing here needs a GPU."""
import math

import numpy as np
import pytest

import branch_cases as BC
import polyline_cases as PC
import topology_cases as TC


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(PC.cases()))
def test_the_walk_and_the_jump_form_agree(name):
    topo, bl, rank, diag, _ = PC.expected(name)
    for n in range(topo.shape[0]):
        r, d = PC.walk(topo[n], bl[n])
        assert np.array_equal(r, rank[n]) and np.array_equal(d, diag[n])
        longest = PC.longest_chain(topo[n], bl[n])
        assert PC.jump_form(topo[n], bl[n])[2] <= PC.rounds_bound(longest)
        P = int(BC.is_branch(topo[n]).sum())
        fixed = PC.jump_form(topo[n], bl[n], rounds=math.ceil(math.log2(P)) if P > 1 else 0)         # the device's round count
        assert np.array_equal(fixed[0], rank[n]) and np.array_equal(fixed[1], diag[n])
        # rank is a position: 0 .. px - 1 within every ordered branch, -1 at every pixel that is no branch pixel
        assert ((rank[n] >= 0) <= (bl[n] != 0)).all() and ((rank[n] < 0) == (diag[n] < 0)).all() and (diag[n] <= rank[n]).all()
        for lab in np.unique(bl[n][rank[n] >= 0]):
            assert sorted(rank[n][bl[n] == lab].tolist()) == list(range(int((bl[n] == lab).sum())))


def test_the_serpentines_need_their_rounds():
    """one path through every tile seam, no junction pixel: 16 964 pixels in 15 rounds (an odd count) and 4 322 in 13"""
    for name, px, rounds in (("serpentine_130x260", 16964, 15), ("serpentine_66x130", 4322, 13)):
        topo, bl, rank, diag, got = PC.expected(name)
        assert not BC.is_junction(topo).any() and int((bl != 0).sum()) == px and len(np.unique(bl[bl != 0])) == 1
        assert got == rounds and rank.max() == px - 1 and (diag[rank >= 0] == 0).all()
        assert rank[0, 0, 0] == 0 and rank[0, 0, 1] == 1                             # from the first row's first pixel eastwards
    assert 2 ** 13 < 16964


def test_hand_values():
    topo, bl, rank, diag, _ = PC.expected("hand_run7")
    assert rank[0, 4, 2:9].tolist() == list(range(7)) and (diag[0, 4, 2:9] == 0).all() and (rank >= 0).sum() == 7
    topo, bl, rank, diag, _ = PC.expected("hand_diag7")
    ys, xs = zip(*sorted(TC.HAND["diag7"][0]))
    assert rank[0, ys, xs].tolist() == list(range(7)) and np.array_equal(rank, diag)
    # the square ring starts at its top-left pixel and goes E first
    topo, bl, rank, diag, _ = PC.expected("hand_ring")
    assert rank[0, 2, 3] == 0 and rank[0, 2, 4] == 1 and rank[0, 3, 3] == 15 and rank[0, 6, 7] == 8 and (diag[rank >= 0] == 0).all()
    # the diamond starts at its top pixel and goes SW first; every link is diagonal
    topo, bl, rank, diag, _ = PC.expected("hand_diamond")
    assert rank[0, 2, 5] == 0 and rank[0, 3, 4] == 1 and rank[0, 3, 6] == 7 and rank[0, 6, 5] == 4 and np.array_equal(rank, diag)
    # the full frame of borders() is one cycle of 402
    topo, bl, rank, diag, _ = PC.expected("borders")
    assert (rank[2] >= 0).sum() == 402 and rank[2].max() == 401 and rank[2, 0, 0] == 0 and rank[2, 0, 1] == 1 and rank[2, 1, 0] == 401
    # the staircase: a diagonal link every second step
    topo, bl, rank, diag, _ = PC.expected("staircase")
    assert rank.max() == 8 and diag.max() == 4 and sorted(diag[rank >= 0].tolist()) == [0, 0, 1, 1, 2, 2, 3, 3, 4]
    # one branch pixel between two junction pixels: a branch of one pixel, rank 0
    topo, bl, rank, diag, _ = PC.expected("pixel_between_junctions")
    assert BC.is_junction(topo)[0, 4, 4] and BC.is_junction(topo)[0, 4, 6] and bl[0, 4, 5] == 4 * 11 + 5 + 1
    assert rank[0, 4, 5] == 0 and diag[0, 4, 5] == 0 and (bl[0] == bl[0, 4, 5]).sum() == 1
    # the ring and the diamond on the corner of four tiles
    topo, bl, rank, diag, _ = PC.expected("corner_rings")
    assert rank[0, 61, 125] == 0 and rank[0, 61, 126] == 1 and (rank[0] >= 0).sum() == 24 and diag[0].max() == 0
    assert rank[1, 60, 128] == 0 and rank[1, 61, 127] == 1 and (rank[1] >= 0).sum() == 16 and np.array_equal(rank[1], diag[1])


def test_swapped_planes_swap_their_results():
    a, b = PC.expected("swapped_ab"), PC.expected("swapped_ba")
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x[0], y[1]) and np.array_equal(x[1], y[0]) and not np.array_equal(x[0], x[1])


def test_a_branch_that_is_no_chain_lies_on_a_plane_with_a_quad():
    seen = 0
    for name in PC.cases():
        topo, bl, rank, _, _ = PC.expected(name)
        for n in range(topo.shape[0]):
            if ((bl[n] != 0) & (rank[n] < 0)).any():
                seen += 1
                assert (topo[n] & TC.QUAD).any(), name
    assert seen > 5


ORDERED_SHARE = 0.96


def test_the_crack_skeletons_are_ordered_but_for_one_branch_a_plane():
    """per plane of ``cracks``: 1 of 77, 0 of 79 and 1 of 88 branches are no chains, with 22, 0 and 21 of 545, 817 and 671 branch pixels --
    95.96 %, 100 % and 96.87 % ordered; over each case as a whole 97.9 %"""
    want = {"cracks": [(77, 1, 545, 22), (79, 0, 817, 0), (88, 1, 671, 21)]}
    for name in ("cracks", "cracks_pruned"):
        topo, bl, rank, _, _ = PC.expected(name)
        total = ordered = 0
        for n in range(topo.shape[0]):
            labs = np.unique(bl[n][bl[n] != 0])
            bad = [lab for lab in labs if rank[n].ravel()[lab - 1] < 0]
            px, lost = int((bl[n] != 0).sum()), int(((bl[n] != 0) & (rank[n] < 0)).sum())
            print(name, n, len(labs), len(bad), px, lost, 1 - lost / px)
            assert len(bad) <= 1
            if name in want:
                assert (len(labs), len(bad), px, lost) == want[name][n]
            total, ordered = total + px, ordered + px - lost
        assert ordered / total >= ORDERED_SHARE


# ------------------------------------------------------------------------------------------------ the host helpers
def test_arc_position_and_the_names():
    from csbsr_amd.utils import estimate_metrics as M
    assert M.ORDER_COLUMNS == PC.ORDER_COLUMNS
    assert M.arc_position(6, 0) == 6.0 and type(M.arc_position(6, 0)) is float and M.arc_position(6, 6) == 6 * PC.SQRT2
    assert M.arc_position(np.int32(5), np.int32(2)) == PC.arc_of(5, 2) == 3 + 2 * PC.SQRT2
    got = M.arc_position(np.array([0, 1, 2, 3]), np.array([0, 0, 1, 2]))
    assert got.dtype == np.float64 and got.tolist() == [PC.arc_of(r, d) for r, d in ((0, 0), (1, 0), (2, 1), (3, 2))]


def test_polyline_stats_on_hand_made_points():
    from csbsr_amd.utils import estimate_metrics as M
    run = np.array([(4, x) for x in range(2, 9)])
    assert M.polyline_stats(run) == dict(start=(4, 2), stop=(4, 8), arc_px=6.0, chord_px=6.0, tortuosity=1.0, direction_deg=0.0)
    up = run[::-1, ::-1]                                                             # a column walked upwards folds to 90 degrees
    assert M.polyline_stats(up)["direction_deg"] == 90.0 and M.polyline_stats(run[::-1])["direction_deg"] == 0.0
    anti = np.array([(d, 6 - d) for d in range(7)])                                  # towards SW: 135 degrees
    s = M.polyline_stats(anti)
    assert s["arc_px"] == 6 * PC.SQRT2 and s["direction_deg"] == 135.0 and abs(s["tortuosity"] - 1.0) < 1e-15
    ell = np.array([(0, 0), (1, 0), (2, 0), (3, 0), (3, 1), (3, 2), (3, 3)])
    s = M.polyline_stats(ell)
    assert s["arc_px"] == 6.0 and s["chord_px"] == math.sqrt(18.0) and s["tortuosity"] == 6.0 / math.sqrt(18.0) and s["direction_deg"] == 45.0
    one = M.polyline_stats(np.array([(3, 4)]))
    assert one == dict(start=(3, 4), stop=(3, 4), arc_px=0.0, chord_px=0.0, tortuosity=None, direction_deg=None)
    none = M.polyline_stats(np.zeros((0, 4), np.int32))
    assert none == dict(start=None, stop=None, arc_px=0.0, chord_px=0.0, tortuosity=None, direction_deg=None)
    ring = np.array([(0, 0), (0, 1), (1, 1), (1, 0)])
    assert M.polyline_stats(ring, cycle=True)["tortuosity"] is None and M.polyline_stats(ring)["tortuosity"] == 3.0
    four = np.array([(0, 0, 0, 9), (1, 1, 1, 4), (1, 2, 1, 0)])                      # rows of branch_polylines: y and x first
    assert M.polyline_stats(four)["arc_px"] == 1 + PC.SQRT2 and M.polyline_stats(four)["stop"] == (1, 2)
    with pytest.raises(ValueError):
        M.polyline_stats(np.array([1, 2, 3]))


@pytest.mark.parametrize("name", ["cracks", "corner_rings", "staircase", "borders", "hand_single", "noise_0.3"])
def test_polyline_stats_equal_the_restatement(name):
    from csbsr_amd.utils import estimate_metrics as M
    topo, bl, rank, diag, _ = PC.expected(name)
    seen = 0
    for n in range(topo.shape[0]):
        chain, offsets, points = PC.polylines_of(bl[n][None], rank[n][None], diag[n][None], BC.fake_d2(bl[n])[None])
        labs = np.unique(bl[n][bl[n] != 0])
        cycles = PC.cycles_of(topo[n], bl[n])
        assert len(labs) == len(chain) == len(offsets) - 1 and offsets[-1] == len(points) == (rank[n] >= 0).sum()
        for j, lab in enumerate(labs):
            pts = points[offsets[j]:offsets[j + 1]]
            cyc = int(lab) in cycles
            assert M.polyline_stats(pts, cycle=cyc) == PC.stats_of(pts, cyc)
            if chain[j]:
                seen += 1
                assert pts.shape[0] == (bl[n] == lab).sum() and (bl[n][pts[:, 0], pts[:, 1]] == lab).all()
                assert np.array_equal(M._diag_along(pts), pts[:, 2])                 # the diagonal steps along the points are the diag column
                assert np.abs(np.diff(pts[:, :2], axis=0)).max(initial=0) <= 1       # consecutive points are neighbours
                assert M.polyline_stats(pts)["arc_px"] == M.arc_position(pts.shape[0] - 1, pts[-1, 2])
    assert seen > 0


def test_a_cycle_is_a_chain_with_as_many_inner_links_as_pixels():
    """predict_dataset tells a cycle from the branch row: links - attach == px (a path has px - 1 inner links).  The kind does not tell: on
    noise a closed chain can carry attach links and count as 'terminal' or 'self_loop'"""
    kinds = set()
    for name in PC.cases():
        topo, bl, rank, _, _ = PC.expected(name)
        for n in range(topo.shape[0]):
            rows = BC.rows_of(topo[n][None], jlabels=None, blabels=bl[n][None])
            cycles = PC.cycles_of(topo[n], bl[n])
            for row, kind in zip(rows.tolist(), BC.kinds_of(rows)):
                r = dict(zip(BC.COLUMNS, row))
                if rank[n].ravel()[r["label"] - 1] >= 0:
                    cyc = r["label"] in cycles
                    assert (r["h"] + r["v"] + r["d_se"] + r["d_sw"] - r["attach"] == r["px"]) == cyc, (name, n, r["label"])
                    if cyc:
                        kinds.add(kind)
    assert "ring" in kinds and len(kinds) > 1


def _branch_lists(with_width):
    """(name, branches) per plane of ``cracks`` with the polyline keys, built by crack_polylines from the restatement's tables"""
    from csbsr_amd import inference as I
    topo, bl, rank, diag, _ = PC.expected("cracks")
    W = topo.shape[2]
    out = []
    for n in range(topo.shape[0]):
        d2 = BC.fake_d2(bl[n]) if with_width else None
        rows = BC.rows_of(topo[n][None], d2=None if d2 is None else d2[None])
        blist = I.crack_branches(rows, W)
        chain, offsets, points = PC.polylines_of(bl[n][None], rank[n][None], diag[n][None], None if d2 is None else d2[None])
        assert I.crack_polylines(blist, chain, points, widths=with_width) is None
        want = PC.polyline_dicts(topo[n], bl[n], rank[n], diag[n], d2)
        assert len(want) == len(blist)
        for b, w in zip(blist, want):
            for key in ("chain", "start", "stop", "arc_px", "chord_px", "tortuosity", "direction_deg"):
                assert b[key] == w[key] and type(b[key]) is type(w[key]), key
            assert b["points"].dtype == np.int32 and np.array_equal(b["points"], w["points"]) and b["points"].shape == (b["px"] if b["chain"] else 0, 2)
            assert ("width_profile_px" in b) == with_width
            if with_width:
                assert b["width_profile_px"].dtype == np.float64 and np.array_equal(b["width_profile_px"], w["width_profile_px"])
        out.append((f"img_{n}.png", blist))
    return out


@pytest.mark.parametrize("with_width", [False, True])
def test_the_csv_file_round_trips(tmp_path, with_width):
    from csbsr_amd import inference as I
    from csbsr_amd.utils import estimate_metrics as M
    rows = _branch_lists(with_width)
    path = str(tmp_path / "crack_polylines.csv")
    I.write_crack_polylines(path, rows)
    got = I.read_crack_polylines(path)
    assert [name for name, _ in got] == [name for name, _ in rows]
    for (_, branches), (_, back) in zip(rows, got):
        kept = [(j, b) for j, b in enumerate(branches) if b["points"].shape[0]]
        assert [d["branch"] for d in back] == [j for j, _ in kept] and all(b["chain"] for _, b in kept)
        for (j, b), d in zip(kept, back):
            assert d["points"].dtype == np.int32 and np.array_equal(d["points"], b["points"])
            assert np.array_equal(d["s_px"], np.atleast_1d(M.arc_position(np.arange(b["px"]), M._diag_along(b["points"])))) and d["s_px"][-1] == b["arc_px"]
            assert ("width_px" in d) == with_width and (not with_width or np.array_equal(d["width_px"], b["width_profile_px"]))
    import skeleton_cases as SC
    assert SC.read_csv(path)[0] == I.POLYLINE_CSV_COLUMNS + (I.POLYLINE_CSV_OPTIONAL if with_width else [])
    with open(path, "w") as fh:
        fh.write("name,branch,y,x\n")
    with pytest.raises(ValueError):
        I.read_crack_polylines(path)


def test_crack_polylines_refuses_points_that_do_not_fit():
    from csbsr_amd import inference as I
    branches = [dict(px=3, kind="free", links=(2, 0, 0, 0), attach=0)]
    with pytest.raises(ValueError):
        I.crack_polylines(branches, [1], np.zeros((4, 4), np.int32))
    with pytest.raises(ValueError):
        I.crack_polylines(branches, [1, 0], np.zeros((3, 4), np.int32))


def test_predict_dataset_refuses_a_bad_polylines_argument_before_the_model_runs():
    from csbsr_amd.inference import predict_dataset
    model = lambda *a, **kw: pytest.fail("the model ran")
    t = 0.4
    for kwargs in (dict(polylines=True), dict(measure_threshold=t, polylines=True), dict(measure_threshold=t, topology=True, polylines=True),
                   dict(measure_threshold=t, topology=True, branches=False, polylines=True),
                   dict(measure_threshold=t, topology=True, branches=True, polylines=1),
                   dict(measure_threshold=t, topology=True, branches=True, polylines=None),
                   dict(measure_threshold=t, topology=True, branches=True, polylines="True")):
        with pytest.raises(ValueError):
            next(predict_dataset(model, None, **kwargs))


def test_the_device_entries_refuse_what_is_no_device_tensor():
    import torch
    from csbsr_amd.utils import estimate_metrics as M
    for bad in (np.zeros((1, 4, 4), np.int32), torch.zeros(1, 4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            M.order_branches(bad, torch.zeros(1, 4, 4, dtype=torch.uint8))
        with pytest.raises(ValueError):
            M.branch_polylines(bad, bad, bad)
