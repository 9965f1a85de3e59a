"""The case tables of tests/step_tail_cases.py, checked without a GPU: every builder proves its exactness claims on the reference (the
proofs run inside the builders, so building a row IS the proof), the rounded optimiser rows hold an honest float32 evaluation
inside their counted bounds (four times inside where the count allows it: _margin), every reference mutant fails the comparison of the rows it applies to -- the SAME comparison
functions tests/test_step_tail_exact_gpu.py applies to the device's output -- the tables reach every size, instance and wrap the kernels
distinguish, and every entry point and kernel of csrc/multi_tensor.hip and every entry point of csrc/image_ops.hip is accounted for."""
import numpy as np
import pytest

import step_tail_cases as S

f32 = np.float32


def _caught(fn, *args):
    """the comparison must reject the mutant's output"""
    with pytest.raises(AssertionError):
        fn(*args)


def test_constants_parse_and_tables_cross_the_seams():
    k = S.constants()
    assert k == dict(CHUNK=8192, BLOCK=256, CAP=8192)
    CH = k["CHUNK"]
    assert set(S.SIZES) >= {0, 1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 3} and max(S.SIZES) > 2 * CH
    assert {n % 4 for n in S.SIZES if 0 < n < CH} == {0, 1, 3} and S.unaligned_n() > CH
    assert [S.head1_ppb(c) for c in S.HEAD1_C] == [32, 16, 8]
    assert [S.head1_wrap_npix(c) for c in S.HEAD1_C] == [262177, 131089, 65545]
    for c in S.HEAD1_C:          # the wrap rows take a second turn of the grid-stride loop, no other row does
        assert S.head1_wrap_npix(c) * (c // 8) > k["BLOCK"] * k["CAP"] >= max(S.head1_npix(c)) * (c // 8)
    assert S.HEAD1B_WRAP[1] * (S.HEAD1B_WRAP[0] // 8) > k["BLOCK"] * k["CAP"] and S.sigb_wrap_npix() == 8192 * 256 + 3


# ------------------------------------------------------------------------------------------- chunk map

@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("order", S.ORDERS)
def test_block_map(kind, order):
    sizes = S.opt_sizes(kind)
    idx, bt, bc = S.block_map(sizes, order)
    CH = S.constants()["CHUNK"]
    assert sorted(idx) == list(range(len(sizes))) and (idx[0] == 0) == (order == "forward")
    want = sorted((r, c) for r, t in enumerate(idx) for c in range((sizes[t] + CH - 1) // CH))
    blocks = sorted(zip(bt.tolist(), bc.tolist()))
    past = [b for b in blocks if b[1] * CH >= sizes[idx[b[0]]]]
    assert sorted(set(blocks) - set(past)) == want and len(past) == 2 and len(blocks) == len(want) + 2
    assert {sizes[idx[r]] - c * CH for r, c in past} == {0, CH + 1 - 5 * CH}          # nothing left, and a negative remainder
    natural = [b for r, t in enumerate(idx) for b in [(r, c) for c in range((sizes[t] + CH - 1) // CH)]]
    assert list(zip(bt.tolist(), bc.tolist()))[:len(natural)] != natural          # permuted
    assert (S.stepped(sizes, idx, bt, bc) == 1).all()                            # every element exactly once
    twice = S.stepped(sizes, idx, bt, bc, tail_twice=True)
    assert int((twice == 2).sum()) == sum(1 for r, c in set(blocks) - set(past) if min(sizes[idx[r]] - c * CH, CH) % 4)
    moved = S.stepped(sizes, idx, bt, bc, chunk1_base=CH - 4)
    assert int((moved == 2).sum()) == sum(min(n - CH, 4) for n in sizes if n > CH) == int((moved == 0).sum())


# ------------------------------------------------------------------------------------------- SGD

def _margin(used, n, what):
    """An honest float32 evaluation (every operation rounded once, nothing fused) against the counted bounds of a rounded row.  ``used``:
    its worst error / bound per output.  Where the count reaches MARGIN x MARGIN roundings the evaluation has to sit MARGIN times
    inside.  Below that it CANNOT: the one rounding of the result alone is up to 2^-24 of the result -- 1 / n of the bound where the terms
    do not cancel -- and the conversions of the hyper-parameters (float32(0.001) is off by 0.8 x 2^-24) come on top: the evaluation uses
    up to 2.7 of the n = 4 .. 9 roundings these rows count.  A larger n would be a bound fitted to pass this check; the counts stay as
    counted, and what is asserted for them is that the evaluation is inside its bound and uses less than MARGIN roundings' worth."""
    for name, r in used.items():
        assert r <= 1.0
        if n[name] >= S.MARGIN * S.MARGIN:
            assert r * S.MARGIN <= 1.0, f"{what} {name}: a float32 evaluation is not {S.MARGIN:g} times inside the bound ({r:.3g})"
        else:
            assert r * n[name] < S.MARGIN, f"{what} {name}: a float32 evaluation uses {r * n[name]:.3g} of the {n[name]} roundings counted"


def _sgd_rows(kind=None):
    return [r for r in S.rows() if r["entry"] == "csbsr_sgd_step" and (kind is None or r["kind"] == kind)]


def test_sgd_rows_cover_the_issue():
    exact = _sgd_rows("exact")
    assert {r["instance"] for r in exact} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(r["instance"], r["order"]) for r in exact} == {(i, o) for i in {r["instance"] for r in exact} for o in S.ORDERS}
    assert all(r["steps"] == (2 if r["weight_decay"] else 4) and r["lr"] == 2.0 ** -3 for r in exact)
    assert {r["momentum"] for r in exact} == {0.0, 0.5} and {r["weight_decay"] for r in exact} == {0.0, 2.0 ** -4}
    (rounded,) = _sgd_rows("rounded")
    assert (rounded["lr"], rounded["momentum"], rounded["weight_decay"]) == (1e-2, 0.9, 5e-4) and rounded["n"] == S.SGD_N
    assert len(_sgd_rows("empty")) == 1 and [(r["momentum"] < 0, r["weight_decay"] < 0) for r in _sgd_rows("refused")] == [(True, False), (False, True)]


@pytest.mark.parametrize("row", _sgd_rows("exact"), ids=lambda r: f"mom{r['momentum']}-wd{r['weight_decay']}-{r['order']}")
def test_sgd_exact_rows(row):
    d = S.sgd_row_case(row)          # (the proofs of every intermediate run in here)
    assert (d["p"] == 0).any() and (d["g"][0] == 0).any() and np.abs(d["p"]).max() == 1.0
    # fused or not: a float32 evaluation step by step gives the reference's bits
    p, b = d["p"], d["buf"]
    for g in d["g"]:
        p, b = S.sgd32(p, b, g, row["lr"], row["momentum"], row["weight_decay"])
    S.sgd_compare(row, p, b)
    for m in S.SGD_MUTANTS:
        if S.sgd_mutant_applies(m, row):
            _caught(S.sgd_compare, row, *S.sgd_mutant(m, row))


def test_sgd_three_steps_with_decay_would_round():
    d = S.sgd_inputs("exact", 2)
    with pytest.raises(AssertionError, match="not fp32-exact"):
        S.sgd_ref(d["p"], d["buf"], d["g"] + d["g"][:1], 2.0 ** -3, 0.5, 2.0 ** -4, prove="three steps")


def test_sgd_rounded_row():
    (row,) = _sgd_rows("rounded")
    d = S.sgd_row_case(row)
    p, b = S.sgd32(d["p"], d["buf"], d["g"][0], row["lr"], row["momentum"], row["weight_decay"])
    used = S.sgd_compare(row, p, b)          # inside the bound: worst error / bound 0.25 (p) and 0.38 (buf)
    _margin(used, S.SGD_N, "sgd")
    for m in S.SGD_MUTANTS:
        _caught(S.sgd_compare, row, *S.sgd_mutant(m, row))


# ------------------------------------------------------------------------------------------- Adam

def _adam_rows(kind=None):
    return [r for r in S.rows() if r["entry"] == "csbsr_adam_step" and (kind is None or r["kind"] == kind)]


@pytest.mark.parametrize("row", _adam_rows("exact"), ids=lambda r: r["order"])
def test_adam_exact_rows(row):
    d = S.adam_case("exact")          # (the proofs of every product run in here)
    assert row["betas"] == (0.5, 0.75) and row["eps"] == 2.0 ** -10 and row["steps"] == 3 == len(d["g"])
    assert all(np.log2(v) == round(np.log2(v)) for t in d["table"] for v in t) and len(set(d["table"])) > 3
    # v still 0 after step 1 where g was 0: denom == eps; and a zero g later, where v is not 0
    assert ((d["g"][0] == 0) & (d["g"][1] == 0)).any() and ((d["g"][0] != 0) & (d["g"][1] == 0)).any()
    # the final update fused into one multiply-add gives the same bits: step_size q is exact
    b1, b2 = row["betas"]
    fused = S.adam32(d["p"], d["m"], d["v"], d["g"], d["step_size"], d["bc2_sqrt"], b1, b2, row["eps"], fused_update=True)
    S.adam_compare(row, *fused)
    for m in S.ADAM_MUTANTS:
        _caught(S.adam_compare, row, *S.adam_mutant(m, row))


def test_adam_six_steps_would_stay_exact():
    d = S.adam_case("exact")
    n = d["p"].size
    gs = d["g"] + [S.lat((n,), 5, 31, (n, 40 + s), 0.75) for s in range(3)]
    S.adam32(d["p"], d["m"], d["v"], gs, d["step_size"], d["bc2_sqrt"], 0.5, 0.75, 2.0 ** -10, prove="six steps")


def test_adam_rounded_row():
    (row,) = _adam_rows("rounded")
    d = S.adam_case("rounded")
    b1, b2 = row["betas"]
    assert d["table"][0] == (2e-5 / (1.0 - 0.9 ** 3), (1.0 - 0.999 ** 3) ** 0.5) and row["eps"] == 1e-8 and row["n"] == S.ADAM_N
    got = S.adam32(d["p"], d["m"], d["v"], d["g"], d["step_size"], d["bc2_sqrt"], b1, b2, row["eps"])
    used = S.adam_compare(row, *got)          # inside the bound: worst error / bound 0.062 (p), 0.54 (m), 0.45 (v)
    _margin(used, S.ADAM_N, "adam")
    for m in S.ADAM_MUTANTS:
        _caught(S.adam_compare, row, *S.adam_mutant(m, row))


def test_fma32_rounds_once():
    a, b, c = f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12), f32(-1.0)
    assert S.fma32(np.array([a]), np.array([b]), np.array([c]))[0] == f32(2.0 ** -11 + 2.0 ** -24) != a * b + c
    # a tie of the fp64 sum that the residual breaks: 1 + 2^-24 (+ 2^-60) rounds UP in one rounding, to even (down) in two
    x = S.fma32(np.array([f32(2.0 ** -30)]), np.array([f32(2.0 ** -30)]), np.array([1.0 + 2.0 ** -24]))
    assert x[0] == f32(1 + 2.0 ** -23)


def test_wrapper_cases():
    sgd, adam = S.wrap_case("sgd"), S.wrap_case("adam")          # (SGD: three steps with decay proved exact in here)
    assert [S.wrap_has_grad(1, s) for s in range(3)] == [True, False, True] and adam[1]["t"] == 2 and adam[0]["t"] == 3
    assert len(adam[0]["ref_p_any"]) == 8 and any((adam[0]["ref_p_any"][0] != c).any() for c in adam[0]["ref_p_any"][1:])
    lag = S.sgd_ref(sgd[1]["p"], np.zeros(S.WRAP_SIZES[1]), sgd[1]["g"], **S.WRAP_SGD)
    assert (lag[0] != sgd[1]["ref_p"]).any()          # a parameter stepped without a gradient shows


# ------------------------------------------------------------------------------------------- head1_fwd

def _head_rows(entry):
    return [r for r in S.rows() if r["entry"] == entry and "refused" not in r]


def test_head1_fwd_rows_cover_the_issue():
    rows = _head_rows("csbsr_head1_fwd")
    for c in S.HEAD1_C:
        mine = [r for r in rows if r["c"] == c]
        small = {(r["split"], r["layout"], r["bias"], r["npix"], r["sigmoid"]) for r in mine if not r["wrap"]}
        assert small == {(s, l, b, n, g) for s in (0, 1) for l in S.LAYOUTS for b in (0, 1) for n in S.head1_npix(c) for g in (0, 1)}
        assert {(r["npix"], r["sigmoid"]) for r in mine if r["wrap"]} == {(S.head1_wrap_npix(c), 0), (S.head1_wrap_npix(c), 1)}
    assert {r["kernels"][0] for r in rows} == {"head1_fwd_kernel<8>", "head1_fwd_kernel<16>", "head1_fwd_kernel<32>"}
    assert [(r["refused"], r["c"], r["ld"]) for r in S.rows() if r["entry"] == "csbsr_head1_fwd" and "refused" in r] == [("c", 32, 32), ("ld", 64, 56)]
    # the counted sigmoid bound implies the 2e-6 absolute bound of test_one_channel_head_kernels
    assert float(S.head1_sigmoid_n(S.HEAD1_T_MAX)) * S.U * 1.0 < 2e-6


def _sigmoid32(t):
    """an honest float32 sigmoid: exp2 of the rounded product with log2(e), the add, the division"""
    t = t.astype(f32)
    e = np.exp2((-t * f32(1.4426950408889634)).astype(np.float64)).astype(f32)
    return f32(1.0) / (f32(1.0) + e)


@pytest.mark.parametrize("c", S.HEAD1_C)
def test_head1_fwd_rows(c):
    used = set()
    for row in [r for r in _head_rows("csbsr_head1_fwd") if r["c"] == c]:
        ref, bound = S.head1_ref(row)          # (the proofs run in head1_case)
        t = S.head1_ref(dict(row, sigmoid=0))[0]
        S.head1_compare(row, _sigmoid32(t) if row["sigmoid"] else t.astype(f32))          # an honest float32 evaluation passes
        if row["sigmoid"]:
            assert (bound > 0).all() and (bound < 2e-6).all()
        for m in S.HEAD1_MUTANTS:
            if S.head1_mutant_applies(m, row):
                used.add(m)
                _caught(S.head1_compare, row, S.head1_mutant(m, row))
    assert used == set(S.HEAD1_MUTANTS)


# ------------------------------------------------------------------------------------------- head1_bwd_input

def test_head1_bwd_input_rows():
    rows = _head_rows("csbsr_head1_bwd_input")
    small = {(r["c"], r["dpre_ld"], r["layout"], r["npix"], r["weights"]) for r in rows if not r["wrap"]}
    assert small == {(c, d, l, n, w) for c in S.HEAD1B_C for d in (8, 16) for l in S.LAYOUTS for n in (1, 33) for w in ("lattice", "random")}
    assert {(r["c"], r["npix"]) for r in rows if r["wrap"]} == {(256, 65541)}
    assert [r["c"] for r in S.rows() if r["entry"] == "csbsr_head1_bwd_input" and "refused" in r] == [12]
    caught = 0
    for row in rows:
        d = S.head1b_case(row["c"], row["npix"], row["weights"])          # (the range of every product is asserted in here)
        S.head1b_compare(row, d["ref"])
        assert d["ref"].shape == (row["npix"], row["c"]) and (row["npix"] == 1 or ((d["ref"] == 0).any() and (d["ref"] != 0).any()))
        for m in S.HEAD1B_MUTANTS:
            if S.head1b_mutant_applies(m, row):
                caught += 1
                _caught(S.head1b_compare, row, S.head1b_mutant(m, row))
    assert caught >= len(rows) // 2


# ------------------------------------------------------------------------------------------- sigmoid_bwd_to_nhwc8

def test_sigmoid_bwd_rows():
    rows = _head_rows("csbsr_sigmoid_bwd_to_nhwc8")
    assert {(r["npix"], r["scale"]) for r in rows} == {(n, s) for n in (1, 255, 257, S.sigb_wrap_npix()) for s in (1.0, 0.125, 0.3)}
    for row in rows:
        d = S.sigb_case(row["npix"], row["scale"])
        if row["npix"] > 1:
            assert {0.0, 1.0, 0.5} <= set(d["p"][:3].tolist()) and (d["dp"] == 0).any()
        assert (d["ref"][:, 1:].view(np.uint16) == 0).all()          # +0.0 bits
        S.sigb_compare(row, d["ref"])          # the float32 restatement is inside the fp64 bound
        for m in S.SIGB_MUTANTS:
            if S.sigb_mutant_applies(m, row):
                _caught(S.sigb_compare, row, S.sigb_mutant(m, row))
    assert {S.sigb_case(1, s)["p"][0] for s in S.SIGB_SCALES} == {0.0, 1.0, 0.5}


# ------------------------------------------------------------------------------------------- coverage

def test_every_row_names_its_entry_and_kernels():
    for r in S.rows():
        assert r["entry"].startswith("csbsr_") and isinstance(r["kernels"], list)
    for file in ("multi_tensor.hip", "image_ops.hip"):
        assert S.source_names(file)
    known = {n for file in ("multi_tensor.hip", "image_ops.hip") for part in S.source_names(file) for n in part}
    assert S._named(S.rows()) <= known, f"rows name what the sources do not have: {sorted(S._named(S.rows()) - known)}"
    assert set(S.COVERED_ELSEWHERE) | set(S.ELSEWHERE) | set(S.NOT_COVERED) <= known
    assert not (S._named(S.rows()) & (set(S.COVERED_ELSEWHERE) | set(S.ELSEWHERE) | set(S.NOT_COVERED))), "a name with rows is listed as covered elsewhere"


def test_every_entry_point_and_kernel_is_accounted_for():
    assert S.missing_names() == []
    assert S.missing_entries() == []
    for name, why in S.NOT_COVERED.items():
        assert len(why.split()) >= 6, f"{name}: a reason, please"
    for table in (S.COVERED_ELSEWHERE, S.ELSEWHERE):
        for name, filename in table.items():
            text = S.names_in_test_file(filename)
            want = name if name.startswith("csbsr_") else name[:-len("_kernel")]          # (a kernel: by the name of what it computes)
            assert want in text, f"{name}: tests/{filename} does not name it"


@pytest.mark.parametrize("entry", sorted({r["entry"] for r in S.rows()}))
def test_coverage_check_notices_a_row_that_leaves(entry):
    without = [r for r in S.rows() if r["entry"] != entry]
    gone = S.missing_names(table=without) + S.missing_entries(table=without)
    assert entry in gone, f"no ledger check notices that {entry} lost its rows"


def test_coverage_check_notices():
    grown = "\n__global__ __launch_bounds__(256) void brand_new_kernel(float* p) {}\nextern \"C\" int csbsr_brand_new(float* p) { return 0; }\n"
    assert S.missing_names(text=S.source("multi_tensor.hip") + grown) == ["csbsr_brand_new", "brand_new_kernel"]
    assert S.missing_entries(text=S.source("image_ops.hip") + grown) == ["csbsr_brand_new"]
    assert set(S.missing_names(elsewhere={})) == {"csbsr_fingerprint", "fingerprint_kernel"}
    assert "csbsr_sdf" in S.missing_entries(elsewhere={}) and len(S.missing_entries(elsewhere={})) == len(S.ELSEWHERE)
    assert S.missing_entries(elsewhere={}, not_covered={"csbsr_sdf": "a reason of at least six words here"}).count("csbsr_sdf") == 0
    assert "not_a_name_anywhere" not in S.names_in_test_file("test_trainer_dp_gpu.py")
