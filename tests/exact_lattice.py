"""Exact-lattice operands for the convolution kernel tests (a plain helper module: tests/test_conv_exact_gpu.py imports it).

Every operand is a small integer times a power of two.  A product of two such values is an integer multiple of the product's unit,
and a sum of such multiples is exact in fp32, in ANY order, while the sum of the terms' magnitudes stays below 2^24 units.  So a
kernel that adds the right terms has no legitimate rounding left: its fp32 accumulator holds the exact value, and the fp16 store of
that value is exact too when the value fits fp16's 11 significant bits.  The test can then ask for ``torch.equal``: any dropped,
repeated or misplaced term shows up, however small.

The helpers draw such operands and PROVE the bounds on the reference before a test relies on them.  A draw that breaks a bound
fails with a message that names the bound, so that a bad table row can neither pass nor fail by accident.
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
