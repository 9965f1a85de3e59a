"""The local crack width without a device: the restatement of tests/width_cases.py against a brute-force double loop and against the form the
kernel takes, the exact widths of straight bars, the host functions of utils/estimate_metrics (width_from_d2, summarize_width_hist,
centerline_px_at_least, width_radius), the CSV writers and readers of inference.py, and the identity that lets predict_dataset measure the
kept cracks against the whole region."""
import math

import numpy as np
import pytest
import torch

import components_cases as CC
import skeleton_cases as SC
import width_cases as WC


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("seed,shape,density,r", [(0, (12, 12), 0.8, 3), (1, (9, 12), 0.95, 2), (2, (12, 7), 0.6, 128), (3, (1, 12), 0.7, 5),
                                                 (4, (12, 1), 0.7, 1), (5, (11, 11), 0.99, 4)])
def test_the_definition_equals_a_double_loop(seed, shape, density, r):
    region = np.random.default_rng(seed).random(shape) < density
    want = WC.d2_brute(region, r)
    assert np.array_equal(WC.d2_of(region, r), want)
    assert (want[~region] == 0).all() and (want[region] >= 1).all() and want.max() <= r * r + 1
    if seed in (1, 5):
        assert (want == r * r + 1).any(), "the case saturates"


def test_planes_without_background_and_single_pixels():
    for shape in ((1, 1), (3, 4), (12, 12)):
        for r in (1, 7, 128):
            assert (WC.d2_of(np.ones(shape, bool), r) == r * r + 1).all() and (WC.d2_brute(np.ones(shape, bool), r) == r * r + 1).all()
            assert (WC.d2_of(np.zeros(shape, bool), r) == 0).all()


def test_the_exact_distance_cases_sit_on_the_edge_of_saturation():
    for r in (1, 5, 33, 64, 128):
        d2, hist = WC.expected(f"exact_r{r}", r)
        assert d2.max(axis=(1, 2)).tolist() == [r * r, r * r + 1]
        assert hist[0, r * r] == 1 and hist[0].sum() == 1 and hist[1, r * r + 1] == 1 and hist[1].sum() == 1


@pytest.mark.parametrize("kind", ["h", "v"])
def test_straight_bars_have_their_width_on_the_centerline(kind):
    """odd widths w give exactly w, even widths w - 1: the centerline lies on one of the two middle rows"""
    planes, sk, t, _ = WC.cases()[f"bars_{kind}"]
    d2, _ = WC.expected(f"bars_{kind}", 64)
    for w, d, s in zip(WC.BAR_WIDTHS, d2, sk):
        got = {WC.width(int(v)) for v in d[s != 0]}
        assert s.sum() > 50 and got == {float(w if w % 2 else w - 1)}, (w, got)


@pytest.mark.parametrize("name,r", [("cracks", 5), ("cracks", 128), ("noise_0.3", 33), ("disk40_corner", 33), ("disk40_corner", 128), ("disk70", 64),
                                    ("four_borders", 64), ("last_columns", 33), ("exact_r64", 64), ("exact_r128", 128), ("ones", 1), ("5x7", 128),
                                    ("skeleton_outside", 5), ("pair_special_values", 64)])
def test_the_kernels_form_equals_the_definition(name, r):
    planes, sk, t, _ = WC.cases()[name]
    want, _ = WC.expected(name, r)
    for p, s, w in zip(planes, sk, want):
        assert np.array_equal(WC.kernel_form(SC.binarise(p, t), s, r), w)


def test_the_cases_cover_what_they_are_for():
    c = WC.cases()
    assert WC.expected("disk70", 64)[1][0, -1] > 0 and WC.expected("disk40_corner", 33)[1][0, -1] > 0                # saturated centres
    assert WC.expected("disk40_corner", 64)[1][0, -1] == 0
    assert (WC.expected("ones", 5)[1][0, -1] == c["ones"][1].sum()) and c["ones"][1].sum() > 0
    assert WC.expected("skeleton_outside", 5)[1][0, 0] > 100 and WC.expected("1x1_clear", 1)[1].tolist() == [[1, 0, 0]]
    d2, _ = WC.expected("last_columns", 5)
    assert (d2[0, :, -1] == 9).all() and SC.SHAPE[1] % 32 != 0                      # not the 1 a background bit past W would give
    d2, _ = WC.expected("four_borders", 64)
    assert d2.max() <= 9 + 4                               # the cross is 5 and 3 wide: the borders do not narrow it, and nothing saturates
    assert not np.isfinite(c["pair_special_values"][0]).all()
    assert c["batch5"][0].shape[0] == 5


# ------------------------------------------------------------------------------------------------ the host functions
def test_width_from_d2():
    from csbsr_amd.utils.estimate_metrics import width_from_d2
    assert width_from_d2(0) == 0.0 and width_from_d2(1) == 1.0 and width_from_d2(4) == 3.0 and width_from_d2(25) == 9.0
    assert type(width_from_d2(2)) is float and width_from_d2(2) == 2.0 * math.sqrt(2.0) - 1.0
    a = width_from_d2(np.array([[0, 1], [9, 16385]]))
    assert a.dtype == np.float64 and a.tolist() == [[0.0, 1.0], [5.0, 2.0 * math.sqrt(16385.0) - 1.0]]
    t = width_from_d2(torch.tensor([0, 4, 5], dtype=torch.int32))
    assert isinstance(t, np.ndarray) and t.tolist() == [0.0, 3.0, 2.0 * math.sqrt(5.0) - 1.0]


def _hist(values, r):
    return np.bincount(np.asarray(values, np.int64), minlength=r * r + 2)


def _same_summary(got, want):
    """the ranks and counts exactly; the mean, an fp64 sum of n <= 1000 positive terms in another order, to n 2^-53 <= 1.2e-13 relative"""
    assert set(got) == set(want)
    for k in want:
        assert got[k] == (pytest.approx(want[k], rel=2e-13, abs=0) if k == "centerline_width_px" else want[k]), k
    return True


def test_summarize_width_hist_on_hand_made_histograms():
    from csbsr_amd.utils.estimate_metrics import centerline_px_at_least, summarize_width_hist
    r = 3                                                  # bins 0 .. 10, 10 = saturated
    # 20 values: the median is rank 9, p95 rank ceil(19) - 1 = 18
    values = [1] * 9 + [4] * 9 + [9, 10]
    got = summarize_width_hist(_hist(values + [0, 0, 0], r), r)
    assert got == {"centerline_px": 20, "outside_px": 3, "saturated_px": 1, "centerline_width_px": pytest.approx((9 * 1.0 + 9 * 3.0 + 5.0 + WC.width(10)) / 20, rel=2e-13, abs=0),
                   "median_width_px": 3.0, "p95_width_px": 5.0, "max_width_px": WC.width(10)}
    assert _same_summary(got, WC.summary(values + [0, 0, 0], r))
    # 21 values: median rank 10, p95 rank ceil(19.95) - 1 = 19
    values = [1] * 10 + [2] * 9 + [5, 8]
    got = summarize_width_hist(torch.from_numpy(_hist(values, r)).to(torch.int32), r)
    assert got["median_width_px"] == WC.width(2) and got["p95_width_px"] == WC.width(5) and got["max_width_px"] == WC.width(8)
    assert got["saturated_px"] == 0 and got["outside_px"] == 0 and _same_summary(got, WC.summary(values, r))
    assert all(type(got[k]) is float for k in ("centerline_width_px", "median_width_px", "p95_width_px", "max_width_px"))
    assert all(type(got[k]) is int for k in ("centerline_px", "outside_px", "saturated_px"))
    # one value; everything saturated; nothing; only pixels outside the region
    assert summarize_width_hist(_hist([4], r), r) == WC.summary([4], r)
    got = summarize_width_hist(_hist([10] * 7, r), r)
    assert got["saturated_px"] == 7 and got["median_width_px"] == got["max_width_px"] == got["centerline_width_px"] == WC.width(10)
    for values in ([], [0, 0]):
        got = summarize_width_hist(_hist(values, r), r)
        assert got == {"centerline_px": 0, "outside_px": len(values), "saturated_px": 0, "centerline_width_px": 0.0, "median_width_px": 0.0,
                       "p95_width_px": 0.0, "max_width_px": 0.0}
    rng = np.random.default_rng(3)
    for n in (1, 2, 19, 20, 21, 100, 101, 1000):
        values = rng.integers(0, 5 * 5 + 2, size=n).tolist()
        assert _same_summary(summarize_width_hist(_hist(values, 5), 5), WC.summary(values, 5))
    # the length of crack at least that wide
    h = _hist([0, 1, 1, 4, 4, 4, 9, 10], r)
    assert [centerline_px_at_least(h, w) for w in (0.0, 1.0, 1.5, 3.0, 3.01, 5.0, WC.width(10), 6.0)] == [7, 7, 5, 5, 2, 2, 1, 0]
    with pytest.raises(ValueError):
        summarize_width_hist(_hist([1], 4), r)             # the histogram of another radius
    with pytest.raises(ValueError):
        summarize_width_hist(np.zeros((2, 11), np.int64), r)


def test_width_radius_refuses_what_it_should():
    from csbsr_amd.utils.estimate_metrics import width_radius
    assert width_radius(1) == 1 and width_radius(128) == 128 and width_radius(np.int64(64)) == 64 and type(width_radius(np.int32(5))) is int
    for bad in (0, -1, 129, True, False, np.bool_(True), 5.0, np.float32(5), "5", None, [5]):
        with pytest.raises(ValueError, match="width_radius"):
            width_radius(bad, "width_radius")


# ------------------------------------------------------------------------------------------------ the files
def test_the_csv_files_round_trip(tmp_path):
    from csbsr_amd import inference as I
    rows = [("a.png", dict(centerline_px=20, saturated_px=1, centerline_width_px=2.0 * math.sqrt(2.0) - 1.0, median_width_px=3.0,
                           p95_width_px=0.1 + 0.2, max_width_px=WC.width(4097), widest=(3, 17))),
            ("b.png", dict(centerline_px=0, saturated_px=0, centerline_width_px=0.0, median_width_px=0.0, p95_width_px=0.0, max_width_px=0.0,
                           widest=None))]
    path = str(tmp_path / "crack_widths.csv")
    I.write_crack_widths(path, rows)
    assert SC.read_csv(path)[0] == I.WIDTH_COLUMNS == ["name", "centerline_px", "saturated_px", "centerline_width_px", "median_width_px",
                                                       "p95_width_px", "max_width_px", "y_widest", "x_widest"]
    assert I.read_crack_widths(path) == rows
    inst = [("a.png", [dict(max_width_px=2.0 * math.sqrt(5.0) - 1.0, widest=(0, 0)), dict(max_width_px=0.0, widest=None)]),
            ("c.png", [dict(max_width_px=9.0, widest=(69, 132))])]
    path = str(tmp_path / "crack_instance_widths.csv")
    I.write_crack_instance_widths(path, inst + [("empty.png", [])])
    assert SC.read_csv(path)[0] == I.INSTANCE_WIDTH_COLUMNS == ["name", "crack", "max_width_px", "y_widest", "x_widest"]
    assert I.read_crack_instance_widths(path) == inst
    assert I.INSTANCE_COLUMNS == ["name", "crack", "y", "x", "area_px", "length_px", "mean_width_px", "y0", "x0", "y1", "x1"]
    with pytest.raises(ValueError):
        I.read_crack_widths(path)
    with pytest.raises(ValueError):
        I.read_crack_instance_widths(str(tmp_path / "crack_widths.csv"))


# ------------------------------------------------------------------------------------------------ kept cracks against the whole region
@pytest.mark.parametrize("density", [0.2, 0.3, 0.45, 0.6])
@pytest.mark.parametrize("min_px", [2, 5, 20])
def test_distances_against_the_region_are_the_distances_against_the_kept_cracks(density, min_px):
    """R the region, K its 8-connected components of at least min_px pixels.  For p in K, the nearest pixel outside K is never closer than
    the nearest pixel outside R: a removed pixel q lies in another component, two components never touch, so the segment from q to p passes
    a background pixel that is no farther.  (The identity is about 8-connectivity: under 4-connectivity diagonal neighbours may belong to
    two components.)"""
    region = CC.noise(density)
    kept = CC.keep(CC.canonical_labels(region, 8)[None], min_px)[0].astype(bool)
    assert 0 < kept.sum() < region.sum()
    for r in (2, 64):
        assert np.array_equal(WC.d2_of(region, r)[kept], WC.d2_of(kept, r)[kept])
