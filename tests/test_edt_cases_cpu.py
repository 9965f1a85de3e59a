"""tests/edt_cases.py validated without a GPU: the references agree with each other on every row of the geometry table, the model of the
device's block-bounded row search reproduces the exact squared distances, every mutant of edt_cases.MUTANTS is caught by the rows named
for it through the comparison functions tests/test_edt_exact_gpu.py uses, and the table covers every width and geometry class.

The bound under which sdf_restated32 (float32) is held to oracle.csbsr_oracle.compute_sdf (float64) is counted in edt_cases' docstring:
3 * 2^-24 + 2^-44 where H^2 + W^2 < 2^24 (a root, the maximum's root, a division; the subtraction has a zero operand), 5 * 2^-24 + 2^-44
beyond (two more for the rounded squares and sums under each root).  Measured here: worst error / bound 0.65 on the exact rows
(big_5x96x1000), 0.20 on the others (the restatement rounds d2 once there, the device up to twice: the GPU test prints the device's)."""
import os

import numpy as np
import pytest

import crack_weight_cases as CW
import edt_cases as E
import step_tail_cases as S

NAMES = [r["name"] for r in E.ROWS]
SMALL = [r["name"] for r in E.ROWS if r["N"] * r["H"] * r["W"] <= 6000]


# ------------------------------------------------------------------------------------------- the references

@pytest.mark.parametrize("name", SMALL)
def test_brute_force_equals_scipy_on_the_small_rows(name):
    fg = E.foreground(E.mask_of(name))[:, 0]
    for f in fg:
        assert np.array_equal(E.d2_brute(f), E.d2_exact(f)) and np.array_equal(E.d2_brute(~f), E.d2_exact(~f))


def test_small_rows_are_many():
    assert len(SMALL) >= 40 and {E.row(n)["cls"] for n in SMALL} >= {"width", "complement", "n3_extents", "all_foreground", "soft", "equal_reach"}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_within_the_counted_bound_of_the_oracle(name):
    res, ref, full = E.refs(name)
    ratio, left = E.sdf_ratio(res, name)
    print(f"MEASURED {name}: float32 restatement against float64, error / bound {ratio:.3f}, pixels left out {left}")
    assert ratio <= 1
    r = E.row(name)
    assert left == (r["H"] * r["W"] * int(full.sum())) and (left > 0) == (name == "all_foreground")
    assert E.sdf_mismatches(res, name) == 0 and not E.sdf_caught(res, name)
    assert np.isnan(ref[full]).all() and (res[full] == -1).all()          # nothing but foreground: NaN in the reference, -1 here
    assert E.sdf_bound(True) == 3 * 2.0 ** -24 + 2.0 ** -44 and E.sdf_bound(False) == 5 * 2.0 ** -24 + 2.0 ** -44


def test_foreground_rule_is_the_reference_truncation():
    v = np.asarray(E.SOFT_VALUES + (0.0, 255.99, 0.999999), np.float32).reshape(1, 1, 1, -1)
    assert E.foreground(v).reshape(-1).tolist() == [False, False, True, True, True, False, False, False, True, False]
    m = E.mask_of("soft_values")
    assert not E.foreground(m)[1].any() and (m[1] != 0).sum() >= m[1].size - 1          # the all-soft sample: no foreground by the rule
    assert (E.refs("soft_values")[0][1] == 0).all() and (E.refs("soft_values")[1][1] == 0).all()
    for v in E.SOFT_VALUES:
        assert (m[0] == np.float32(v)).any()
    assert np.signbit(m[0]).any() and ((m[0] != 0) & (np.abs(m[0]) < np.finfo(np.float32).tiny)).any()
    assert m.min() >= 0 and m.max() < 256 and m[2].max() > 255


# ------------------------------------------------------------------------------------------- the model of the search

@pytest.mark.parametrize("name", NAMES)
def test_model_without_a_defect_is_exact(name):
    fg = E.foreground(E.mask_of(name))[:, 0]
    assert np.array_equal(E.model_d2(fg), np.stack([E.d2_exact(f) for f in fg]))
    assert np.array_equal(E.model_d2(~fg), np.stack([E.d2_exact(~f) for f in fg]))


@pytest.mark.parametrize("mutant,name", [(m, n) for m, (_, names) in E.MUTANTS.items() for n in names])
def test_every_mutant_is_caught_by_its_rows(mutant, name):
    m = E.mask_of(name)
    got = E.mutant_sdf(m, mutant)
    assert E.sdf_caught(got, name), f"{mutant} ({E.MUTANTS[mutant][0]}) passes the comparisons on {name}"
    if E.row(name)["exact"]:
        assert E.sdf_mismatches(got, name) > 0
    if mutant in E.WEIGHT_MUTANTS:
        w = E.mutant_weight(m, mutant, E.weight_amp(name))
        assert E.weight_caught(w, name), f"{mutant} passes the weight comparison on {name}"


def test_mutant_table_is_complete():
    assert set(E.MUTANTS) == set(E.DEFECTS) | {"batch_max", "eight", "ne0"} and all(names for _, names in E.MUTANTS.values())
    assert set(E.WEIGHT_MUTANTS) == set(E.DEFECTS) | {"ne0"}
    assert not E.sdf_caught(E.mutant_sdf(E.mask_of("n3_extents"), None), "n3_extents")          # no defect, nothing caught
    assert not E.weight_caught(E.mutant_weight(E.mask_of("n3_extents"), None, E.weight_amp("n3_extents")), "n3_extents")
    # the ``!= 0`` rule on a {0, 1} mask is the truncation rule: nothing changes for the masks of every other fixture
    assert E.sdf_mismatches(E.mutant_sdf(E.mask_of("big_5x96x1000"), "ne0"), "big_5x96x1000") == 0


@pytest.mark.parametrize("name", NAMES)
def test_an_error_of_one_in_d2_exceeds_the_weight_bound(name):
    """On every background pixel of a sample with foreground where d2 <= 2^21 (edt_cases.weight_amp): the weight of d2 + 1 and of d2 - 1
    (d2 > 1) misses the bound (amp d + 2) 2^-23 of tests/test_crack_weight_gpu.py; and no reference weight is below FLT_MIN."""
    fg, d, none, amp = E.weight_refs(name)
    assert amp == float(np.float32(amp)) and 0 < amp <= 2
    ref = E.LAMBDA * np.exp(-amp * d)
    assert (ref >= CW.FLT_MIN).all() and amp * d.max() <= 80.001
    d2 = np.rint(d * d)
    crit = ~fg & ~none[:, None, None, None] & (d2 <= E.D2_RESOLVED)
    if not crit.any():
        assert none.all() or fg[~none].all()
        return
    bound = (amp * d[crit] + 2) * 2.0 ** -23
    for delta in (1, -1):
        off = np.maximum(d2[crit] + delta, 0)
        rel = np.abs(E.LAMBDA * np.exp(-amp * np.sqrt(off)) - ref[crit]) / ref[crit]
        assert (rel > bound).all(), f"{name}: an error of {delta} in d2 hides under the bound, worst margin {float((rel / bound).min()):.2f}"
    r = E.row(name)
    if r["cls"] not in ("beyond", "largest", "full_sparse"):
        assert d2.max() <= E.D2_RESOLVED          # the geometry rows are resolved everywhere


# ------------------------------------------------------------------------------------------- coverage

def test_every_width_and_geometry_class_has_a_row():
    assert {r["cls"] for r in E.ROWS} == set(E.CLASSES)
    for W in E.WIDTHS:
        assert {r["H"] for r in E.ROWS if r["cls"] == "width" and r["W"] == W} == set(E.HEIGHTS)
    assert E.WIDTHS == (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 1000) and E.HEIGHTS == (1, 2, 3, 40)
    shapes = {(r["N"], r["H"], r["W"]) for r in E.ROWS}
    assert {(5, 96, 1000), (1, 200, 1000), (1, 3, 4096), (1, 64, 1792)} <= shapes
    assert max(r["N"] * r["H"] * r["W"] for r in E.ROWS) == 5 * 96 * 1000
    for r in E.ROWS:
        assert r["exact"] == (r["H"] ** 2 + r["W"] ** 2 < 2 ** 24) and len(r["why"].split()) >= 6
        assert r["W"] <= E.MAX_W and (r["W"] <= 4096 or r["H"] <= 3)
        assert E.mask_of(r["name"]).shape == (r["N"], 1, r["H"], r["W"])
    assert {r["W"] for r in E.ROWS if not r["exact"]} == {4096, 4097, 8192}
    assert (8192 + 8192 // 32) * 4 < 64 * 1024          # the widest row's LDS
    lone = E.foreground(E.mask_of("lone_feature"))[:, 0]
    assert sorted(int(np.nonzero(s.any(0))[0][0]) for s in lone) == [0, 31, 32, 63, 994, 999] and (lone.reshape(6, -1).sum(1) == 1).all()
    assert E.row("lone_feature")["W"] % 32 != 0 and 994 >= 32 * (999 // 32)
    sparse = E.foreground(E.mask_of("full_sparse")).mean()
    assert 0.002 <= sparse <= 0.006
    seeded = E.mask_of("seeded_sparse")
    assert set(np.unique(seeded[0])) == {0.0, 1.0} and ((seeded[1] > 0) & (seeded[1] < 1)).sum() > 100
    halo = E.mask_of("soft_halo")
    assert set(np.unique(halo)) == {0.0, 0.5, 1.0}
    empty = E.foreground(E.mask_of("empty_cols"))[0, 0].any(0)
    blocks = np.pad(empty, (0, 31)).reshape(-1, 32).any(1)[:17]
    assert blocks.tolist() == [True] + [False] * 9 + [True] + [False] * 6
    n3 = E.foreground(E.mask_of("n3_extents")).reshape(3, -1)
    assert n3[0].sum() == 1 and n3[1].mean() > 0.5 and n3[2].sum() == 0 and E.row("n3_extents")["H"] == 5
    comp = E.foreground(E.mask_of("complement")).reshape(2, -1)
    assert (~comp[0]).sum() == 1 and comp[1].sum() == 1
    full = [r["name"] for r in E.ROWS if E.all_foreground(E.mask_of(r["name"])).any()]
    assert full == ["all_foreground"]


def test_ledger_points_at_the_exact_suite():
    assert S.ELSEWHERE["csbsr_sdf"] == "test_edt_exact_gpu.py"
    with open(os.path.join(S.TESTS, "test_edt_exact_gpu.py")) as f:
        text = f.read()
    assert 'call("csbsr_sdf"' in text and 'call("csbsr_crack_weight"' in text and "pytestmark = pytest.mark.gpu" in text
    assert "csbsr_sdf" in S.names_in_test_file("test_edt_exact_gpu.py")
