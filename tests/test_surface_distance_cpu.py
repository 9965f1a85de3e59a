"""HD / MSD of the evaluation loop, host side (no GPU): the derived contour-length table against the reference's (carried by the fixture
as data), and the fp64 finish -- a function of integer counts keyed by (squared distance, length class) -- against the reference's HD / MSD
on every cell of the fixture, with the counts built here from SciPy's EDT."""
import numpy as np

import surface_cases as S


def test_length_table_matches_reference():
    from csbsr_amd.utils.estimate_metrics import contour_length_table, contour_class_table, CLASS_LENGTH
    g = S.load_fixture()
    t = contour_length_table()
    assert t.shape == (16,) and t.dtype == np.float64
    assert np.abs(t - g["length_table"]).max() <= 1e-15
    assert sorted(set(t.tolist())) == sorted(CLASS_LENGTH.tolist()) and len(set(CLASS_LENGTH.tolist())) == 4
    assert np.all(np.diff(CLASS_LENGTH) > 0)          # class order = length order: bins sort by (d^2, class) like (distance, length)
    assert np.array_equal(contour_class_table() == 0, np.arange(16) % 15 == 0)


def test_finish_from_integer_counts_reproduces_fixture():
    from csbsr_amd.utils.estimate_metrics import surface_metrics_from_counts, contour_class_table
    g = S.load_fixture()
    cls = contour_class_table()
    percent, tie = float(g["percent"]), float(g["tie_margin"])
    for name in g["cases"]:
        prob, mask = S.fixture_inputs(g, name)
        preds = S.binarise(prob, g["thresholds"])
        gt = mask > 0.5
        T = len(preds)
        hd, msd = np.zeros(T), np.zeros(T)
        n_hd = n_msd = 0
        for j in range(T):
            a, b = S.integer_counts(gt, preds[j], cls)
            hd[j], msd[j], ho, mo = surface_metrics_from_counts(a, b, percent, prob.shape[1])
            n_hd += ho
            n_msd += mo
        err, ties = S.compare_case(name, hd, msd, g[f"hd_{name}"], g[f"msd_{name}"], g[f"margin_{name}"], tie)
        print(f"{name}: MSD rel err {err:.2e}, {ties} tie cells skipped for HD")
        assert n_hd == int(g[f"hd_outliers_{name}"]) and n_msd == int(g[f"msd_outliers_{name}"])


def test_fixture_keeps_its_conditions():
    g = S.load_fixture()
    tie = float(g["tie_margin"])
    margins = np.concatenate([g[f"margin_{n}"] for n in g["random_cases"]])
    assert (margins < tie).mean() <= 0.05
    shapes = [g[f"prob_{n}"].shape for n in g["random_cases"]]
    assert any(h != w for h, w in shapes) and any(h % 2 and w % 2 for h, w in shapes)
    assert len(g["thresholds"]) == 99


def test_restatement_agrees_with_fixture():
    """the SciPy restatement the GPU tests lean on (percent 95, full size) is itself pinned to the reference at percent 50"""
    g = S.load_fixture()
    for name in ("rand_61x203", "two_edges", "all_ones"):
        prob, mask = S.fixture_inputs(g, name)
        preds = S.binarise(prob, g["thresholds"])
        r = np.array([S.restate_cell(mask > 0.5, p, g["length_table"], float(g["percent"]), prob.shape[1]) for p in preds])
        S.compare_case(name, r[:, 0], r[:, 1], g[f"hd_{name}"], g[f"msd_{name}"], g[f"margin_{name}"], float(g["tie_margin"]))
        assert np.allclose(r[:, 4], g[f"margin_{name}"], rtol=0, atol=1e-12)
