"""The NumPy restatement of the spur pruning (tests/prune_cases.py) against a second statement of the same rules, against the tiled form the
kernels compute, against the properties a pruning must have and against hand-derived counts; the host helpers of
utils/estimate_metrics.py, the CSV writers and readers of inference.py and predict_dataset's argument checks.  Nothing here needs a GPU."""
import numpy as np
import pytest

import prune_cases as PR
import skeleton_cases as SC

SMALL = [n for n, p in PR.cases().items() if p.shape[1] * p.shape[2] <= 1000]       # the hand shapes, the narrow planes, the batch, ...
SMALL_TILE = dict(th=8, tw=16, kp=2, kg=3, halo_x=4)


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(PR.cases()))
def test_shifted_planes_equal_the_statement_by_pixels(name):
    planes = PR.cases()[name]
    big = planes.shape[1] * planes.shape[2] > 10000
    for plane in planes[:1] if big else planes:
        for L in (3,) if big else (1, 5, 20):
            assert _equal(PR.prune(plane, L), PR.prune_brute(plane, L)), L


@pytest.mark.parametrize("L", [1, 8, 17])
def test_shifted_planes_equal_the_statement_by_pixels_on_the_seam_spurs(L):
    for plane in PR.seam_spurs(L):
        assert _equal(PR.prune(plane, L), PR.prune_brute(plane, L))


@pytest.mark.parametrize("name", ["noise_0.05", "noise_0.3", "noise_0.6", "noise_0.95", "cracks", "seam_shapes", "thin_between_full", "ones"])
def test_the_bit_sliced_adders_give_the_tips(name):
    for plane in PR.cases()[name]:
        assert np.array_equal(PR.tips_adder_form(plane), PR.tips_of(plane)[0])


def test_the_cap_on_the_neighbours_is_what_keeps_outlines_and_removes_stubs():
    """the last pixel of a spur on a straight run has three neighbours and is a tip; a pixel of a thick region's straight outline has five and
    is none"""
    t = PR.hand("T_19_3")
    tips = PR.tips_of(PR.prune(t, 2)[1])[0]                                         # two steps: one spur pixel is left, under the run
    assert tips[5, 14] and PR.prune(t, 3)[0][5, 14] == 0
    assert not PR.tips_of(np.ones((6, 9), np.uint8))[0][[0, -1], 1:-1].any()


# ------------------------------------------------------------------------------------------------ tile by tile
@pytest.mark.parametrize("name,Ls", [("cracks", (9, 64)), ("seam_shapes", (4, 17)), ("long_spur", (18, 33, 64)), ("noise_0.3", (2, 9)),
                                     ("noise_65x129", (8, 17)), ("corners", (5, 33))])
def test_the_tiled_form_equals_the_global_one_at_the_kernels_sizes(name, Ls):
    for plane in PR.cases()[name]:
        for L in Ls:
            assert _equal(PR.tiled(plane, L), PR.prune(plane, L)), L


@pytest.mark.parametrize("L", [7, 8, 9, 17, 18])
def test_the_tiled_form_equals_the_global_one_on_the_seam_spurs(L):
    for plane in PR.seam_spurs(L):
        assert _equal(PR.tiled(plane, L), PR.prune(plane, L))


@pytest.mark.parametrize("name", SMALL)
def test_the_tiled_form_equals_the_global_one_with_many_seams(name):
    """tiles of 8 x 16 with two peel and three grow steps per launch: every shape lies across several seams"""
    for plane in PR.cases()[name]:
        for L in (1, 2, 3, 4, 7, 12):
            assert _equal(PR.tiled(plane, L, **SMALL_TILE), PR.prune(plane, L)), L


# ------------------------------------------------------------------------------------------------ what a pruning must do
@pytest.mark.parametrize("density", PR.DENSITIES)
def test_the_five_properties_on_noise(density):
    for seed in (0, 1):
        plane = PR.noise(density, (40, 50), seed)
        for L in (1, 2, 4, 9, 20):
            PR.properties_hold(plane, L)
        skel = SC.skeleton(plane)
        for L in (1, 2, 4, 9, 20):
            PR.properties_hold(skel, L)


@pytest.mark.parametrize("seed", PR.CRACK_SEEDS)
def test_the_five_properties_on_the_crack_skeletons(seed):
    removed = [PR.properties_hold(PR.crack_skeleton(seed), L) for L in (1, 4, 8, 16, 64)]
    assert removed == sorted(removed) == list(PR.FIXTURE_REMOVED[seed].values())


# ------------------------------------------------------------------------------------------------ by hand
@pytest.mark.parametrize("name", list(PR.HAND))
def test_hand_shapes_lose_their_hand_derived_pixels(name):
    plane = PR.hand(name)
    for L, want in PR.HAND[name][1].items():
        out, xl, t = PR.prune(plane, L)
        assert int(plane.sum() - out.sum()) == want, L
        assert t.max() <= L and ((t > 0) == ((plane != 0) & (xl == 0))).all()


def test_what_goes_is_the_spur_and_the_short_arm():
    t = PR.hand("T_19_3")
    gone = np.argwhere((t != 0) & (PR.prune(t, 3)[0] == 0))
    assert gone.tolist() == [[5, 14], [6, 14], [7, 14]]
    f = PR.hand("fork_5_3")
    gone = np.argwhere((f != 0) & (PR.prune(f, 10)[0] == 0))
    assert gone.tolist() == [[11, 23], [12, 24], [13, 25]]                          # the arm of 3 that runs down; the arm of 5 comes back whole
    r = PR.hand("ring_tail")
    assert (PR.prune(r, 11)[0] == r).all() and PR.prune(r, 12)[0].sum() == 28 and PR.holes(PR.prune(r, 64)[0]) == 1


def test_the_fixture_counts_and_the_tips_that_are_left():
    sk = PR.crack_skeleton(0)
    assert int(PR.tips_of(sk)[0].sum()) == PR.FIXTURE_TIPS_0[0]
    for seed in PR.CRACK_SEEDS:
        for L, want in PR.FIXTURE_REMOVED[seed].items():
            out = PR.prune(PR.crack_skeleton(seed), L)[0]
            assert int(PR.crack_skeleton(seed).sum() - out.sum()) == want
            if seed == 0:
                assert int(PR.tips_of(out)[0].sum()) == PR.FIXTURE_TIPS_0[L]


def test_the_documented_biases():
    """a real branch of up to L pixels off a loop goes; of two unequal arms the shorter goes when it is at most L long; on a plane that is
    not thin only corner-like pixels go"""
    assert int(PR.hand("ring_tail").sum() - PR.prune(PR.hand("ring_tail"), 12)[0].sum()) == 12
    f = PR.hand("fork_5_3")
    assert int(f.sum() - PR.prune(f, 2)[0].sum()) == 0 and int(f.sum() - PR.prune(f, 3)[0].sum()) == 3
    thick = np.zeros((20, 30), np.uint8)
    thick[4:15, 5:25] = 1
    out = PR.prune(thick, 64)[0]
    assert thick.sum() - out.sum() <= 4 and out[5:14, 6:24].all()


def test_the_seam_cases_sit_on_the_seams():
    for L in (1, 9, 64):
        s = PR.seam_spurs(L)
        assert s[:, :, 127].any() and s[:, :, 128].any() and s[:, 63].any() and s[:, 64].any()
        assert PR.prune_of(s, L)[2].tolist() == [2 * max(L - 1, 1), 2 * L, 0]
    a, b, c = PR.seam_shapes()
    assert a[64, 128] and b[63:65, 127:129].all() and c[63, 20] and c[64, 20] and c[10, 127] and c[10, 128]
    assert PR.long_spur()[0, 11:51, 100].all() and PR.long_spur()[0, 72, 110:150].all() and PR.prune_of(PR.long_spur(), 39)[2].tolist() == [0] and PR.prune_of(PR.long_spur(), 40)[2].tolist() == [80]
    assert PR.spur_lengths() == (1, 2, 7, 8, 9, 17, 18, 33, 64)


# ------------------------------------------------------------------------------------------------ the host helpers
def test_spur_length():
    from csbsr_amd.utils import estimate_metrics as M
    assert M.PRUNE_MAX_SPUR == PR.MAX_SPUR == 64
    assert M.spur_length(1) == 1 and M.spur_length(64) == 64 and type(M.spur_length(np.int32(7))) is int
    for bad in (0, 65, -3, True, False, np.bool_(True), 4.0, np.float32(4), "4", None, [4]):
        with pytest.raises(ValueError, match="spur_px"):
            M.spur_length(bad)
    with pytest.raises(ValueError, match="prune_spur_px"):
        M.spur_length(0, "prune_spur_px")


# ------------------------------------------------------------------------------------------------ the files
def test_the_csv_files_round_trip(tmp_path):
    from csbsr_amd import inference as I
    rows = [("a.png", 812, 11), ("b.png", 0, 0)]
    path = str(tmp_path / "crack_spurs.csv")
    I.write_crack_spurs(path, rows)
    assert SC.read_csv(path)[0] == I.SPUR_COLUMNS == ["name", "skeleton_px", "spur_px"]
    assert I.read_crack_spurs(path) == rows
    inst = [("a.png", [dict(length_px=40, spur_px=3), dict(length_px=0, spur_px=0)]), ("c.png", [dict(length_px=7, spur_px=12)])]
    ipath = str(tmp_path / "crack_instance_spurs.csv")
    I.write_crack_instance_spurs(ipath, inst + [("empty.png", [])])
    assert SC.read_csv(ipath)[0] == I.INSTANCE_SPUR_COLUMNS == ["name", "crack", "length_px", "spur_px"]
    assert I.read_crack_instance_spurs(ipath) == inst
    with pytest.raises(ValueError):
        I.read_crack_spurs(ipath)
    with pytest.raises(ValueError):
        I.read_crack_instance_spurs(path)


# ------------------------------------------------------------------------------------------------ the driver's argument checks
def test_predict_dataset_refuses_a_bad_prune_spur_px_before_the_model_runs():
    from csbsr_amd.inference import predict_dataset
    model = lambda *a, **kw: pytest.fail("the model ran")
    for kwargs in (dict(prune_spur_px=4), dict(prune_spur_px=4, topology=False), dict(measure_threshold=0.4, prune_spur_px=0),
                   dict(measure_threshold=0.4, prune_spur_px=65), dict(measure_threshold=0.4, prune_spur_px=-1), dict(measure_threshold=0.4, prune_spur_px=True),
                   dict(measure_threshold=0.4, prune_spur_px=False), dict(measure_threshold=0.4, prune_spur_px=4.0), dict(measure_threshold=0.4, prune_spur_px="4"),
                   dict(measure_threshold=0.4, prune_spur_px=np.bool_(True)), dict(measure_threshold=0.4, topology=True, prune_spur_px=2.5)):
        with pytest.raises(ValueError, match="prune_spur_px"):
            next(predict_dataset(model, None, **kwargs))
