"""The NumPy restatement of the crack topology (tests/topology_cases.py) against its own definition and against what it must equal -- a
brute-force double loop, hand-derived counts, closed forms, a flood fill of the background --, the documented biases of the geodesic
length, the host helpers of utils/estimate_metrics.py, the CSV writers and readers of inference.py and predict_dataset's argument checks.
Nothing here needs a GPU."""
import math

import numpy as np
import pytest

import components_cases as CC
import skeleton_cases as SC
import topology_cases as TC


def _counts(plane):
    return dict(zip(TC.COLUMNS, (int(k) for k in TC.counts_of(TC.topo_of(plane)))))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", [f"hand_{k}" for k in TC.HAND] + ["framed_batch", "noise_5x7", "noise_1x12", "noise_12x1", "ones_5x7", "ones_1x1"])
def test_shifted_planes_equal_the_double_loop(name):
    for plane in TC.cases()[name]:
        assert np.array_equal(TC.topo_of(plane), TC.topo_brute(plane))


@pytest.mark.parametrize("density", [0.1, 0.3, 0.5, 0.7, 0.9])
def test_shifted_planes_equal_the_double_loop_on_noise(density):
    plane = TC.noise(density, (17, 35), 21)
    assert np.array_equal(TC.topo_of(plane), TC.topo_brute(plane))


@pytest.mark.parametrize("name", ["noise_0.05", "noise_0.3", "noise_0.6", "noise_0.95", "ones_5x7", "cracks", "seams", "framed_batch"])
def test_the_bit_sliced_adder_gives_the_classes(name):
    for plane, topo in zip(TC.cases()[name], TC.expected(name)[0]):
        for cls, got in zip((TC.ISOLATED, TC.END, TC.PATH, TC.JUNCTION), TC.adder_form(plane)):
            assert np.array_equal(got, (topo & 7) == cls), cls


def test_the_ring_order_is_what_separates_a_plus_from_a_blob():
    """the centre of a plus has four separate arms: A = 4 by ring adjacency, a junction (Guo-Hall's C(P), which pairs the ring positions,
    does not count four there and cannot be used for the class)"""
    t = TC.topo_of(TC.hand("plus"))
    assert (t[4, 5] & 7) == TC.JUNCTION and sorted((t[t != 0] & 7).tolist()).count(TC.END) == 4


@pytest.mark.parametrize("name", list(TC.HAND))
def test_hand_shapes_have_their_hand_derived_counts(name):
    plane, want = TC.hand(name), TC.HAND[name][1]
    got = _counts(plane)
    got["loops"] = TC.loops_of(plane)
    got["length"] = TC.length(got["h"], got["v"], got["d_se"], got["d_sw"])
    assert {k: got[k] for k in want} == want
    assert got["V"] == len(TC.HAND[name][0]) and got["loops"] == TC.holes(plane)
    assert got["V"] == got["isolated"] + got["end"] + got["path"] + got["junction_px"]


@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_straight_and_diagonal_runs(n):
    run = np.ones((1, n), np.uint8)
    c = _counts(run)
    assert TC.length(c["h"], c["v"], c["d_se"], c["d_sw"]) == n - 1 and _counts(run.T)["v"] == n - 1
    for d in (np.eye(n, dtype=np.uint8), np.eye(n, dtype=np.uint8)[::-1]):
        c = _counts(d)
        assert (c["h"], c["v"], c["d_se"] + c["d_sw"]) == (0, 0, n - 1)
        assert TC.length(c["h"], c["v"], c["d_se"], c["d_sw"]) == TC.SQRT2 * (n - 1)


@pytest.mark.parametrize("h,w", TC.SHAPES + (TC.SHAPE,))
def test_all_ones_and_all_zeros_have_closed_forms(h, w):
    c = _counts(np.ones((h, w), np.uint8))
    assert (c["V"], c["h"], c["v"], c["d_se"], c["d_sw"], c["q4"]) == (h * w, h * (w - 1), (h - 1) * w, 0, 0, (h - 1) * (w - 1))
    assert TC.euler(TC.counts_of(TC.topo_of(np.ones((h, w), np.uint8)))) == 1
    assert not TC.topo_of(np.zeros((h, w), np.uint8)).any()


# ------------------------------------------------------------------------------------------------ loops = enclosed cells
def test_loops_equal_the_flood_fill_on_140_random_planes():
    rng = np.random.default_rng(2)
    seen = set()
    for density in np.linspace(0.05, 0.95, 7):
        for _ in range(20):
            plane = rng.random((17, 19)) < density
            want = TC.holes(plane)
            assert TC.loops_of(plane) == want, density
            seen.add(want)
    assert len(seen) > 5


@pytest.mark.parametrize("seed", TC.CRACK_SEEDS)
def test_loops_of_a_skeleton_are_the_holes_of_its_region(seed):
    region, skel = TC.crack_region(seed), TC.crack_skeleton(seed)
    loops = TC.loops_of(skel)
    assert loops == TC.holes(skel) == TC.holes(region) and loops > 5              # thinning preserves the holes
    assert SC.components(skel) == SC.components(region)
    c = _counts(skel)
    assert 0 < TC.junctions_of(skel) <= c["junction_px"] and c["end"] > 0


@pytest.mark.parametrize("density", [0.05, 0.2, 0.35, 0.5, 0.7, 0.95])
def test_the_link_graph_has_the_components_of_8_connectivity(density):
    plane = TC.noise(density, (23, 41), 9)
    assert TC.link_graph_components(plane) == SC.components(plane)


@pytest.mark.parametrize("name", [n for n in TC.cases() if n.startswith(("seams", "borders", "framed", "two_and_one")) or n in ("noise_0.3", "noise_0.6")])
def test_loops_equal_the_flood_fill_on_the_cases(name):
    for plane, c in zip(TC.cases()[name], TC.expected(name)[1]):
        assert TC.loops_of(plane, c) == TC.holes(plane)


def test_the_seam_cases_sit_on_the_seams():
    s = TC.seams()
    for plane in s[:3]:
        assert plane[63].any() and plane[64].any() and plane[:, 127].any() and plane[:, 128].any() and plane[:, 31].any() and plane[:, 32].any()
    c = TC.expected("seams")[1]
    assert c[0][TC.COLUMNS.index("junction_px")] == 14 and c[0][TC.COLUMNS.index("end")] == 4 * 14
    assert c[1][TC.COLUMNS.index("d_se")] == 6 * 14 and c[2][TC.COLUMNS.index("d_sw")] == 6 * 14
    b = TC.borders()
    assert b[0][0].any() and b[0][-1].all() and b[1][:, 0].any() and b[1][:, -1].all()
    assert [TC.holes(p) for p in b] == [0, 0, 1, 4]


def test_the_framed_batch_would_link_across_planes_if_the_planes_were_one():
    x = TC.framed_batch()
    N, H, W = x.shape
    stacked = TC.counts_of(TC.topo_of(x.reshape(N * H, W)))
    apart = TC.expected("framed_batch")[1].sum(axis=0)
    assert stacked[TC.COLUMNS.index("v")] == apart[TC.COLUMNS.index("v")] + (N - 1) * W


# ------------------------------------------------------------------------------------------------ the documented biases
def test_the_length_bias_of_a_straight_line():
    """the chain-code length of a straight digital line reads long by at most sqrt(1 + (sqrt(2) - 1)^2) - 1 = 8.24 %, reached at 22.5 degrees;
    the pixel count of a 45-degree line reads 1 - 1 / sqrt(2) = 29.3 % short"""
    worst = math.sqrt(1.0 + (math.sqrt(2.0) - 1.0) ** 2)
    assert worst == pytest.approx(1.0824, abs=5e-5)
    ratios = {}
    for angle in (0.0, 5.0, 10.0, 15.0, 20.0, 22.5, 25.0, 30.0, 35.0, 40.0, 45.0):
        img, true = TC.rasterised_line(angle)
        c = _counts(img)
        assert c["end"] == 2 and c["junction_px"] == 0 and TC.loops_of(img) == 0
        ratios[angle] = TC.length(c["h"], c["v"], c["d_se"], c["d_sw"]) / true
        assert 1.0 - 1e-12 <= ratios[angle] <= worst + 1e-12, angle              # the ratio depends on rise / run alone: the bound is never passed
    assert ratios[0.0] == 1.0 and ratios[45.0] == pytest.approx(1.0, abs=1e-12)
    assert max(ratios, key=ratios.get) == 22.5 and ratios[22.5] == pytest.approx(worst, abs=1e-5)
    img, true = TC.rasterised_line(45.0)
    assert 1.0 - (img.sum() - 1) / true == pytest.approx(1.0 - 1.0 / math.sqrt(2.0), abs=1e-12) and 1.0 - 1.0 / math.sqrt(2.0) == pytest.approx(0.293, abs=5e-4)


# ------------------------------------------------------------------------------------------------ the host helpers
def test_host_helpers():
    from csbsr_amd.utils import estimate_metrics as M
    assert M.TOPOLOGY_COLUMNS == TC.COLUMNS and M.TOPOLOGY_TABLE_COLUMNS == TC.ROW_COLUMNS
    assert (M.TOPO_ISOLATED, M.TOPO_END, M.TOPO_PATH, M.TOPO_JUNCTION) == (1, 2, 3, 4)
    assert (M.TOPO_QUAD, M.TOPO_E, M.TOPO_S, M.TOPO_SE, M.TOPO_SW) == (8, 16, 32, 64, 128)
    assert M.geodesic_length(6, 0, 0, 0) == 6.0 and type(M.geodesic_length(6, 0, 0, 0)) is float
    assert M.geodesic_length(0, 0, 6, 0) == 6 * math.sqrt(2.0) and M.geodesic_length(1, 2, 3, 4) == 3 + 7 * math.sqrt(2.0)
    assert M.geodesic_length(0, 0, 0, 0) == 0.0
    got = M.geodesic_length(np.array([1, 0]), np.array([2, 0]), np.array([3, 1]), np.array([4, 0]))
    assert got.dtype == np.float64 and got.tolist() == [3 + 7 * math.sqrt(2.0), math.sqrt(2.0)]
    assert M.orientation_shares(0, 0, 0, 0) == (0.0, 0.0, 0.0, 0.0)
    assert M.orientation_shares(3, 1, 0, 0) == (0.75, 0.25, 0.0, 0.0) and M.orientation_shares(0, 0, 5, 0) == (0.0, 0.0, 1.0, 0.0)
    s = M.orientation_shares(1, 2, 3, 4)
    assert s == TC.shares(1, 2, 3, 4) and sum(s) == pytest.approx(1.0, abs=1e-15) and all(type(k) is float for k in s)
    assert M.euler_number(8, (0, 0, 4, 4), 0) == 0 and M.euler_number(4, (2, 2, 0, 0), 1) == 1 and type(M.euler_number(np.int32(4), [2, 2, 0, 0], 1)) is int
    assert M.mean_width_geodesic(10, 4.0) == 2.5 and M.mean_width_geodesic(10, 0.0) == 0.0 and M.mean_width_geodesic(0, 0.0) == 0.0
    for seed in TC.CRACK_SEEDS:
        skel = TC.crack_skeleton(seed)
        want = TC.summary(skel)
        got = M.summarize_topology(TC.counts_of(TC.topo_of(skel)), SC.components(skel), TC.junctions_of(skel))
        assert {k: got[k] for k in want} == want
        assert got["loops"] == TC.holes(skel) and got["skeleton_px"] == int(skel.sum()) and got["components"] == SC.components(skel)
        assert got["euler"] == got["components"] - got["loops"]
        assert all(type(got[k]) is int for k in ("endpoints", "junctions", "junction_px", "isolated_px", "loops")) and type(got["length_geodesic_px"]) is float
    empty = M.summarize_topology(np.zeros(10, np.int32), 0, 0)
    assert (empty["loops"], empty["length_geodesic_px"], empty["orientation"], empty["links"]) == (0, 0.0, (0.0, 0.0, 0.0, 0.0), (0, 0, 0, 0))
    for bad in (np.zeros(9, np.int32), np.zeros((2, 10), np.int32)):
        with pytest.raises(ValueError):
            M.summarize_topology(bad, 0, 0)


def test_crack_topology_of_one_crack():
    from csbsr_amd import inference as I
    for name in ("square", "T", "diamond", "single", "block"):
        plane = TC.hand(name)
        row = TC.topology_rows(CC.canonical_labels(plane)[None], TC.topo_of(plane)[None])
        assert len(row) == 1
        got = I.crack_topology(row[0, 2:].tolist(), int(plane.sum()))
        assert got == TC.crack_of(row[0, 2:], int(plane.sum())) and got["loops"] == TC.holes(plane)
    assert I.crack_topology([0] * 9, 0)["loops"] == 0                               # a crack whose centerline is empty


# ------------------------------------------------------------------------------------------------ the files
def test_the_csv_files_round_trip(tmp_path):
    from csbsr_amd import inference as I
    rows = [("a.png", dict(endpoints=5, junctions=2, junction_px=3, isolated_px=1, loops=4, links=(10, 7, 3, 2), length_geodesic_px=17 + 5 * math.sqrt(2.0),
                           orientation=TC.shares(10, 7, 3, 2), mean_width_geodesic_px=0.1 + 0.2)),
            ("b.png", dict(endpoints=0, junctions=0, junction_px=0, isolated_px=0, loops=0, links=(0, 0, 0, 0), length_geodesic_px=0.0,
                           orientation=(0.0, 0.0, 0.0, 0.0), mean_width_geodesic_px=0.0))]
    path = str(tmp_path / "crack_topology.csv")
    I.write_crack_topology(path, rows)
    assert SC.read_csv(path)[0] == I.TOPOLOGY_CSV_COLUMNS == ["name", "endpoints", "junctions", "junction_px", "isolated_px", "loops", "h", "v", "d_se",
                                                             "d_sw", "length_geodesic_px", "share_h", "share_v", "share_se", "share_sw",
                                                             "mean_width_geodesic_px"]
    assert I.read_crack_topology(path) == rows
    inst = [("a.png", [dict(endpoints=2, junctions=0, loops=0, links=(0, 0, 6, 0), length_geodesic_px=6 * math.sqrt(2.0), orientation=(0.0, 0.0, 1.0, 0.0)),
                       dict(endpoints=0, junctions=0, loops=1, links=(8, 8, 0, 0), length_geodesic_px=16.0, orientation=(0.5, 0.5, 0.0, 0.0))]),
            ("c.png", [dict(endpoints=3, junctions=1, loops=0, links=(4, 2, 1, 0), length_geodesic_px=6 + math.sqrt(2.0), orientation=TC.shares(4, 2, 1, 0))])]
    ipath = str(tmp_path / "crack_instance_topology.csv")
    I.write_crack_instance_topology(ipath, inst + [("empty.png", [])])
    assert SC.read_csv(ipath)[0] == I.INSTANCE_TOPOLOGY_COLUMNS == ["name", "crack", "endpoints", "junctions", "loops", "h", "v", "d_se", "d_sw",
                                                                   "length_geodesic_px", "share_h", "share_v", "share_se", "share_sw"]
    assert I.read_crack_instance_topology(ipath) == inst
    with pytest.raises(ValueError):
        I.read_crack_topology(ipath)
    with pytest.raises(ValueError):
        I.read_crack_instance_topology(path)


# ------------------------------------------------------------------------------------------------ the driver's argument checks
def test_predict_dataset_refuses_a_bad_topology_argument_before_the_model_runs():
    from csbsr_amd.inference import predict_dataset
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(topology=True), dict(topology=True, min_crack_px=5), dict(measure_threshold=0.4, topology=1), dict(measure_threshold=0.4, topology=0),
                   dict(measure_threshold=0.4, topology=None), dict(measure_threshold=0.4, topology="yes"), dict(measure_threshold=0.4, topology=np.bool_(True)),
                   dict(topology=None), dict(topology=1.0)):
        with pytest.raises(ValueError, match="topology"):
            next(predict_dataset(model, None, **kwargs))
