"""The reference of the split-fp16 convolution rows (tests/split_conv_cases.py) proves its own bounds and tells every mutant apart, on the
CPU: what tests/test_split_conv_exact_gpu.py then asks of the kernels with ``torch.equal`` is neither vacuous nor unreachable."""
import math

import pytest
import torch
import torch.nn.functional as F

import exact_lattice as XL
import split_conv_cases as SC
from conv_exact_cases import DEFAULT_MODES
from split_conv_cases import SPLIT_ROWS

IDS = [r.name for r in SPLIT_ROWS]
FP64_PROOF_MACS = 3e9          # rows up to this many multiply-adds repeat the accumulator in fp64 (the 65536-pixel rows rest on the bound alone)


def _differs(a, b):
    return float((a.double() != b.double()).double().mean())


@pytest.mark.parametrize("row", SPLIT_ROWS, ids=IDS)
def test_bounds_hold(row):
    """build() asserts them all (the pack emulation, the product bound, the lattice, fp32-exact steps, fp16-normal planes); here: the span it
    measured, the accumulator again in fp64 and as the sum of separately computed products"""
    c = SC.build(row)
    assert 1.0 <= c.span < XL.FP32_EXACT, f"{row.name}: span 2^{SC.span_log2(c):.1f} units"
    print(f"{row.name}: sum of |terms| bound 2^{SC.span_log2(c):.2f} units of 2^{math.log2(c.unit):g}")
    if row.op == "dgrad":
        assert c.ref.dtype == torch.float16 and tuple(c.ref.shape) == (row.N, c.cseg, row.H, row.W)
        return
    assert c.hi.dtype == c.lo.dtype == torch.float16 and tuple(c.hi.shape) == (row.N, row.cout, c.OH, c.OW)
    # hi + lo carries the value: |t - (hi + lo)| is at most half an fp16 ulp of lo
    err = (c.t.double() - c.hi.double() - c.lo.double()).abs()
    assert bool((err <= c.lo.double().abs() * 2.0 ** -11).all()), f"{row.name}: hi + lo is not the value to lo's rounding"
    xs, ws = SC._plan_operands(c, row.plan)
    parts = sum(SC._conv(row, x, w).double() for x, w in zip(xs, ws))
    assert torch.equal(parts, c.pre.double()), f"{row.name}: the concatenated convolution is not the sum of its products: {XL.mismatch(c.pre, parts)}"
    macs = row.N * c.OH * c.OW * row.cout * row.k * row.k * c.csp * len(xs)
    if macs <= FP64_PROOF_MACS:
        pre64 = SC._conv(row, torch.cat(xs, 1).double(), torch.cat(ws, 1).double())
        assert torch.equal(pre64, c.pre.double()), f"{row.name}: the fp32 accumulator is not its fp64 run: {XL.mismatch(c.pre, pre64)}"
        # the sum of |terms| itself (what the bound bounds): the span the kernels' fp32 accumulation has to be exact over
        mags = float(SC._conv(row, torch.cat(xs, 1).double().abs(), torch.cat(ws, 1).double().abs()).max()) / c.unit
        print(f"{row.name}: largest sum of |terms| 2^{math.log2(mags):.2f} units")
        assert mags <= c.span, f"{row.name}: the sum of |terms| 2^{math.log2(mags):.2f} exceeds its bound 2^{SC.span_log2(c):.2f}"
    if row.plan in (2, 5):
        assert bool((c.v_lo != 0).any()), f"{row.name}: no v_lo drawn: the row could not tell a kernel that multiplies it"


@pytest.mark.parametrize("row", SPLIT_ROWS, ids=IDS)
def test_every_mutant_shows(row):
    """each mutant of the reference changes the expected planes (the sums, on the BatchNorm rows) of every row it applies to"""
    c = SC.build(row)
    for m in SC.mutants_of(row):
        if row.op == "dgrad":
            got, _ = SC.expected_dgrad(c, m)
            share = _differs(got, c.ref)
        else:
            hi, lo, _, stat = SC.expected(c, m)
            share = max(_differs(hi, c.hi), _differs(lo, c.lo))
            if c.bn:
                share = max(share, _differs(stat, c.stat))
        print(f"{row.name}: mutant {m} changes {100 * share:.1f} % of the elements")
        assert share > 0, f"{row.name}: mutant {m} leaves the expected output unchanged ({100 * share:.1f} % of the elements differ)"


def test_mutant_sets():
    """every mutant applies somewhere; the general-K mutant to exactly the fused general-K rows; the v_lo mutants to no two-product row"""
    used = {m for r in SPLIT_ROWS for m in SC.mutants_of(r)}
    assert used == set(SC.MUTANTS) | set(SC.DGRAD_MUTANTS)
    gk = [r.name for r in SPLIT_ROWS if "xlo_shift32" in SC.mutants_of(r)]
    assert gk == ["fs_glds64_gk", "fs_glds128_gk", "fs_glds256_gk", "fs_glds256w_gk"]
    for r in SPLIT_ROWS:
        if r.plan in (1, 2, 5):
            assert "no_xhi_wlo" not in SC.mutants_of(r)


def test_rows_are_well_formed():
    names = [r.name for r in SPLIT_ROWS]
    assert len(names) == len(set(names)), "duplicate row names"
    for r in SPLIT_ROWS:
        assert r.op in SC.ENTRY and r.entry == SC.ENTRY[r.op], r.name
        assert r.kid >= 0, f"{r.name}: no kernel ID"
        assert r.why, f"{r.name}: say why the row reaches its kernel"
        assert r.out_c0 and r.out_c0[0] == 0, r.name
        assert (r.plan == 0) == (r.op == "dgrad") and r.blocks in (1, 2, 3) and r.fused in (0, 1), r.name
        if r.op != "dgrad":
            want = {1: (1,), 2: (2, 5), 3: (3, 4)}[r.blocks]
            assert r.plan in want, f"{r.name}: fwd_blocks {r.blocks} cannot run plan {r.plan}"
        for name, _ in r.modes:
            assert name in DEFAULT_MODES, f"{r.name}: mode {name} has no default to restore"
        assert not r.budget or r.kid == 20, f"{r.name}: only the conv_x3n rows walk tiles under a CU budget"
    assert SC.WSCALE == 256.0


def test_the_draws_name_the_bound_they_break():
    g = torch.Generator().manual_seed(1)
    with pytest.raises(AssertionError, match="fp32 bound"):
        XL.assert_products_bound([(1152, 2 * 2.0 ** 9, 2, 2.0 ** 9), (1152, 2 * 2.0 ** -4, 2, 2.0 ** -4), (1152, 2 * 2.0 ** 9, 2.0 ** -12, 2.0 ** -4)], 2.0 ** -4, "dense")
    with pytest.raises(AssertionError, match="no whole multiple"):
        XL.assert_products_bound([(10, 1, 1, 2.0 ** -6)], 2.0 ** -4, "unit")
    with pytest.raises(AssertionError, match="fp16-subnormal"):
        XL.assert_fp16_normal(torch.tensor([0.0, 1.0, 2.0 ** -15]), "plane")
    XL.assert_fp16_normal(torch.tensor([0.0, -2.0 ** -14, 3.0]), "plane")
    with pytest.raises(AssertionError, match="half an ulp"):
        XL.draw_split_weights((4, 4), amp=2, shift=11, gen=g)
    hi, lo = XL.draw_split_planes((2, 8, 5, 5), 9, gen=g)
    assert float(hi.abs().max()) == 2.0 ** 10 and float(lo.abs().max()) == 2.0 ** -3
    v_hi, v_lo = XL.draw_split_weights((64, 64), gen=g)
    assert not bool(((v_lo != 0) & (v_hi == 0)).any()) and bool((v_lo != 0).any())


def test_the_three_products_are_not_the_full_product():
    """the issue's premise: on this lattice the three-product sum differs from the full (hi + lo)(hi + lo) product and from the sum without
    x_hi w_lo in most output elements"""
    c = SC.build(SC.BY_NAME["fs_glds128"])
    full = F.conv2d((c.x_hi + c.x_lo).double(), (c.v_hi + c.v_lo).double(), None, 1, 1)
    two = F.conv2d((c.x_hi + c.x_lo).double(), c.v_hi.double(), None, 1, 1)
    assert _differs(full, c.pre) > 0.9 and _differs(two, c.pre) > 0.9
