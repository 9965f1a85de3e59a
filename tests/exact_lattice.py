"""Exact-lattice operands for the convolution kernel tests (a plain helper module: tests/test_conv_exact_gpu.py imports it).

Every operand is a small integer times a power of two.  A product of two such values is an integer multiple of the product's unit,
and a sum of such multiples is exact in fp32, in ANY order, while the sum of the terms' magnitudes stays below 2^24 units.  So a
kernel that adds the right terms has no legitimate rounding left: its fp32 accumulator holds the exact value, and the fp16 store of
that value is exact too when the value fits fp16's 11 significant bits.  The test can then ask for ``torch.equal``: any dropped,
repeated or misplaced term shows up, however small.

The helpers draw such operands and PROVE the bounds on the reference before a test relies on them.  A draw that breaks a bound
fails with a message that names the bound, so that a bad table row can neither pass nor fail by accident.

The split-fp16 (hi + lo) convolutions sum three products of different units in one accumulator: draw_split_planes / draw_split_weights
draw their operand pairs, assert_products_bound proves the common bound, assert_fp16_normal keeps the output planes out of fp16's
subnormals (tests/split_conv_cases.py).
"""
import math

import torch

FP32_EXACT = 1 << 24          # integers below this are exact in fp32


def draw(shape, q, amp=1, density=0.5, gen=None):
    """integers in [-amp, amp] times 2^-q, zero with probability 1 - density (fp32 CPU tensor); fp16-exact for amp <= 2048"""
    assert 0 < amp <= 2048 and q <= 14
    v = torch.randint(-amp, amp + 1, tuple(shape), generator=gen, dtype=torch.int32)
    keep = torch.rand(tuple(shape), generator=gen) < density
    return (v * keep).to(torch.float32) * 2.0 ** -q


def density_for(k_terms, target=600.0):
    """operand density that keeps a K-term sum of two draws near ``target`` nonzero products (its values then fit fp16)"""
    return min(0.5, math.sqrt(target / max(k_terms, 1)))


def assert_sum_bound(n_terms, max_a, max_b, unit, what):
    """K x max|a| x max|b| < 2^24 units: a summation of n_terms products is exact in fp32 whatever its order"""
    bound = n_terms * float(max_a) * float(max_b) / unit
    assert bound < FP32_EXACT, (f"{what}: the draw breaks the fp32 bound: K * max|a| * max|b| = {bound:.3g} units >= 2^24 "
                                f"(K = {n_terms}); use sparser or smaller operands")


def assert_products_bound(products, unit, what):
    """several products summed in ONE fp32 accumulator (the split-fp16 convolution: x_hi w_hi + x_lo w_hi + x_hi w_lo).  ``products`` is a
    list of (K, max|a|, max|b|, unit of the product): every product's unit is a whole multiple of the common ``unit`` (so every term is
    an integer number of units), and the sum over the products of K x max|a| x max|b| stays below 2^24 units (so any summation order of
    all the terms is exact).  K is the largest number of NONZERO terms of that product in any one sum -- the reference counts them on the
    drawn operands (a convolution of the operands' nonzero masks); the a-priori K of a dense draw would break the bound.  Returns the
    bound in units."""
    total = 0.0
    for n_terms, max_a, max_b, u in products:
        ratio = u / unit
        assert ratio >= 1 and ratio == round(ratio), f"{what}: a product's unit 2^{math.log2(u):g} is no whole multiple of the common unit 2^{math.log2(unit):g}"
        total += n_terms * float(max_a) * float(max_b) / unit
    assert total < FP32_EXACT, (f"{what}: the draw breaks the fp32 bound: sum over the products of K * max|a| * max|b| = {total:.3g} units "
                                f"(2^{math.log2(max(total, 1)):.1f}) >= 2^24; use sparser or smaller operands")
    return total


def draw_split_planes(shape, a, amp=2, density=0.5, shift=13, gen=None):
    """the two planes of a split (hi + lo) map, drawn INDEPENDENTLY (the kernels' contract is plane arithmetic, not canonical pairs):
    hi = i 2^a, lo = j 2^(a - shift), |i|, |j| <= amp, each zero with probability 1 - density; both fp16-exact and fp16-normal"""
    assert -14 <= a - shift and a + math.log2(amp) <= 15, "the planes leave fp16's normal range"
    return draw(shape, 0, amp, density, gen) * 2.0 ** a, draw(shape, 0, amp, density, gen) * 2.0 ** (a - shift)


def draw_split_weights(shape, amp=2, density=0.5, shift=13, gen=None):
    """SCALED weights v = v_hi + v_lo of a split operand: v_hi = k, v_lo = m 2^-shift, |k|, |m| <= amp, v_lo nonzero only where k != 0 --
    so fp16(v) = v_hi and fp16(v - fp16(v)) = v_lo (|v_lo| is below half an fp16 ulp of every nonzero v_hi, asserted).  Returns
    (v_hi, v_lo); the master weight is (v_hi + v_lo) / WSCALE, exact in fp32."""
    assert amp * 2.0 ** -shift < 2.0 ** -11, "v_lo reaches half an ulp of v_hi = 1: fp16(v) would not be v_hi"
    v_hi = draw(shape, 0, amp, density, gen)
    v_lo = draw(shape, 0, amp, 1.0, gen) * 2.0 ** -shift * (v_hi != 0)
    return v_hi, v_lo


def assert_fp16_normal(t, what):
    """every value is zero or at least 2^-14 in magnitude: no fp16-subnormal in an output plane (a store that flushes subnormals and one
    that keeps them would both pass a comparison that never sees one -- and differ on the hardware; the draw's exponent avoids them)"""
    a = t.double().abs()
    bad = (a != 0) & (a < 2.0 ** -14)
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} values are fp16-subnormal (smallest {float(a[bad].min()) if bool(bad.any()) else 0:.3g}): "
                                 f"raise the draw's exponent")


def assert_on_lattice(t, unit, what):
    """every value is an integer multiple of ``unit``: a reference that rounded somewhere (an fp32 algorithm other than a plain sum of
    products) fails here, not in the comparison"""
    r = t.double() / unit
    bad = r != torch.round(r)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} reference values are off the 2^{round(math.log2(unit))} lattice: the reference rounded"


def assert_fp16_exact(t, what):
    """every value fits fp16 (11 significant bits, exponent in range): the kernel's fp16 store of the exact value is exact"""
    td = t.double()
    bad = td.half().double() != td
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} reference values are not fp16-exact (max |r| = {float(td.abs().max()):.6g}): "
                                 f"the draw breaks the fp16 bound; use sparser or smaller operands")


def assert_fp32_exact(t, what):
    td = t.double()
    bad = td.float().double() != td
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} reference values are not fp32-exact"


def assert_sq_sum_bound(v, unit, dims, what):
    """BatchNorm sums: sum of (v / unit)^2 over ``dims`` below 2^24 (the sums of squares are exact then)"""
    m = float(((v.double() / unit) ** 2).sum(dims).max())
    assert m < FP32_EXACT, f"{what}: sum of squares = {m:.3g} units^2 >= 2^24: size the case to fit"


def mismatch(got, ref):
    """one line on where two tensors differ (assertion messages)"""
    g, r = got.double(), ref.double()
    bad = ~((g == r) | (torch.isnan(g) & torch.isnan(r)))
    n = int(bad.sum())
    if n == 0:
        return "identical"
    idx = tuple(int(i) for i in torch.nonzero(bad)[0])
    return f"{n} of {bad.numel()} elements differ ({int(torch.isnan(g).sum())} NaN in the result), first at {idx}: got {float(g[idx])!r}, want {float(r[idx])!r}"
