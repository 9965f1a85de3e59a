"""Shared by tests/test_step_tail_cases_cpu.py and tests/test_step_tail_exact_gpu.py: references, exact-lattice inputs, case tables,
comparisons and reference mutants for the tail of a training step -- the two multi-tensor optimiser steps of csrc/multi_tensor.hip
(csbsr_sgd_step, four template instances; csbsr_adam_step) and the 1-channel head kernels of csrc/image_ops.hip (csbsr_head1_fwd, three
instances; csbsr_head1_bwd_input; csbsr_sigmoid_bwd_to_nhwc8).  No GPU.

References (fp64 numpy unless stated):

  SGD             per element d = g + wd p (skipped when wd == 0); b = mom b + d (skipped when mom == 0); p -= lr b (p -= lr d when
                  mom == 0).  Exact rows: every operand an integer in [-64, 64] x 2^-6, lr = 2^-3, mom = 1/2, wd in {0, 2^-4}; the
                  builder proves with assert_fp32_exact that EVERY intermediate of every step (wd p, d, mom b, b, lr b, p) is fp32-exact,
                  so a fused and an unfused evaluation give the same bits (the device contracts multiply-adds, torch does not).  Two
                  steps with decay, four without (a third step with decay needs 28 bits).
  Adam            a float32 restatement operation by operation in the kernel's order: m + w1 (g - m); v beta2 + (w2 g) g;
                  sqrt(v) / bc2_sqrt + eps; p - step_size (m / denom), w1 = float32(1 - beta1), w2 = float32(1 - beta2) from doubles.
                  Exact rows: beta1 = 1/2, beta2 = 3/4, step_size and bc2_sqrt powers of two set in the table, eps = 2^-10, g integers in
                  [-31, 31] x 2^-5, p on 2^-6: the builder proves in fp64 that every product that feeds an add -- w1 (g - m), v beta2,
                  (w2 g) g, step_size q -- is fp32-exact, so no contraction can change a bit, while sqrt, / and the adds round once each,
                  correctly (fp32 / and sqrtf compile to the correctly rounded sequences).  Three steps.
  rounded rows    the training hyper-parameters on random operands, ONE step from random state, against fp64 under the counted
                  per-element bound |got - ref64| <= n 2^-24 sum|terms| of tests/elementwise_cases.py; n and the terms next to SGD_N / ADAM_N
                  (every rounding counted once, the conversions of the double hyper-parameters to fp32 included).
  head1_fwd       out[px] = sum_c (hi + lo)[px, c] w[c] + bias.  hi on 2^-2 {-3 .. 3}, lo on 2^-8 {-7 .. 7}, w on 2^-4 {-7 .. 7}: hi + lo is
                  exact in fp32, every product is a multiple of 2^-12 and the sum of magnitudes stays below 2^24 units: any fold order
                  gives the same fp32 value t.  sigmoid = 0: bit-equal.  sigmoid = 1: |got - sigmoid64(t)| <= (|t| + 4) 2^-24 sigmoid64(t)
                  (HEAD1_SIGMOID_N), |t| <= 8 asserted.
  head1_bwd_input dx[px, c] = float16(float32(d[px]) w[c]): one correctly rounded fp32 product and a round-to-nearest-even fp16 store;
                  nothing can contract: bit-exact against numpy float32 on lattice and on random fp32 weights.
  sigmoid_bwd     out[i, 0] = float16(((dp p) (1 - p)) scale) in float32 in that order, channels 1 .. 7 +0.0: no multiply feeds an add:
                  bit-exact up to the two things sigb_compare names (the device fuses the product with the scale into the store: one
                  rounding for two; the sign of a zero result); and against fp64 under 3 fp32 roundings + 2^-11 for the store.

Every row is a dict with ``entry`` (the C entry point) and ``kernels`` (the __global__ kernels the call launches); missing_names()
checks csrc/multi_tensor.hip entirely and the extern "C" entry points of csrc/image_ops.hip against the rows, the tables of names
another suite asserts (COVERED_ELSEWHERE / ELSEWHERE) and the written reasons (NOT_COVERED).
"""
import functools
import os
import re

import numpy as np
import torch

from elementwise_cases import H16, LAYOUTS, MARGIN, U, layout  # noqa: F401  (re-exported to the two test modules)
from exact_lattice import assert_fp16_exact, assert_fp32_exact, assert_sum_bound, draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csbsr_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
f32 = np.float32


# ------------------------------------------------------------------------------------------- what the sources state

@functools.lru_cache(maxsize=None)
def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def constants():
    """the chunk size of the multi-tensor kernels and the block size / grid cap of grid_for(), read from the lines that state them: a
    change of one of them changes these numbers (or breaks a pattern) and test_step_tail_cases_cpu.py fails the tables"""

    def one(file, pattern, what):
        m = re.search(pattern, source(file))
        assert m, f"{what}: pattern {pattern!r} not found in csrc/{file}"
        return tuple(int(g) for g in m.groups())

    (CHUNK,) = one("multi_tensor.hip", r"#define CSBSR_MT_CHUNK (\d+)", "multi-tensor chunk")
    BLOCK, CAP = one("image_ops.hip", r"grid_for\(long work, int block = (\d+), int cap = (\d+)\)", "grid cap")
    (HB,) = one("image_ops.hip", r"const long ppb = (\d+) / LPP;", "head1_fwd pixels per block")
    assert HB == BLOCK
    return dict(CHUNK=CHUNK, BLOCK=BLOCK, CAP=CAP)


def _seed(*key):
    h = 1469598103
    for v in key:
        h = (h * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def lat(shape, q, amp, key, density=0.5):
    """float64 numpy lattice draw: integers in [-amp, amp] x 2^-q, zero with probability 1 - density"""
    return draw(shape, q, amp, density, _seed(*key)).double().numpy()


def lat32(shape, q, amp, key, density=0.5):
    """the same as float32 (the large maps of the wrap rows: every lattice value is fp32-exact)"""
    return draw(shape, q, amp, density, _seed(*key)).numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_bits(got, want, what):
    """``got`` holds the bit patterns of ``want`` (same dtype and shape)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype}{got.shape} for {want.dtype}{want.shape}"
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


def check_bound(got, ref, bound, what):
    """|got - ref| <= bound per element, exact where the bound is 0; returns the worst error / bound"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert not np.isnan(err).any(), f"{what}: NaN in the result"
    assert (err[bound == 0] == 0).all(), f"{what}: an element with a zero bound is not exact"
    r = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    assert r <= 1.0, f"{what}: error {r:.4g} x its bound"
    return r


# ------------------------------------------------------------------------------------------- optimisers: tensor list and chunk map

# the vector body alone (4, 8192), the tail alone (1, 3), both (5, 1023, 8191); one chunk, two (8193: a last chunk of 1 element;
# 16387 = 2 x 8192 + 3: three chunks, the last of 3 elements) and three (20000); an empty tensor gets no workgroup
SIZES = (0, 1, 3, 4, 5, 1023, 1028, 8191, 8192, 8193, 16387, 20000)
ORDERS = ("forward", "reversed")          # the order of the table's rows; the per-tensor results must not depend on it


def unaligned_n():
    """SGD's vec = 0 tensor: p, g and buf start 4 bytes into their allocations; two chunks, both through the scalar loop"""
    return constants()["CHUNK"] + 5


def opt_sizes(kind):
    return SIZES + ((unaligned_n(),) if kind == "sgd" else ())


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def split(flat, sizes):
    off = offsets(sizes)
    return [flat[off[i]:off[i + 1]] for i in range(len(sizes))]


def block_map(sizes, order):
    """(idx, block_tensor, block_chunk): table row r holds tensor idx[r]; every chunk of every tensor once, then two blocks whose chunk
    lies past their tensor's end (chunk 1 of the 8192-element tensor: 0 elements remain; chunk 5 of the 8193-element one: the
    remainder is negative) -- they must change nothing -- and the whole list permuted: workgroup order must not matter"""
    CH = constants()["CHUNK"]
    idx = list(range(len(sizes)))
    if order == "reversed":
        idx.reverse()
    bt, bc = [], []
    for r, t in enumerate(idx):
        for c in range((sizes[t] + CH - 1) // CH):
            bt.append(r)
            bc.append(c)
    for n, c in ((CH, 1), (CH + 1, 5)):
        bt.append(idx.index(sizes.index(n)))
        bc.append(c)
    perm = np.random.RandomState(len(bt) + (order == "reversed")).permutation(len(bt))
    return idx, np.array(bt, np.int32)[perm], np.array(bc, np.int32)[perm]


def stepped(sizes, idx, bt, bc, chunk1_base=None, tail_twice=False):
    """how often one launch over the map steps each element of the flat (forward-order) tensor list: the rule of mt_chunk() in
    csrc/multi_tensor.hip -- all ones for a right map.  The keyword arguments are the two positional mutants: chunk 1 based at
    ``chunk1_base`` (its count still taken from the true remainder), and the first element of every scalar tail stepped twice"""
    CH = constants()["CHUNK"]
    off, times = offsets(sizes), np.zeros(int(sum(sizes)), np.int64)
    for r, c in zip(bt, bc):
        t = idx[int(r)]
        cnt = min(max(sizes[t] - int(c) * CH, 0), CH)
        base = chunk1_base if (chunk1_base is not None and c == 1) else int(c) * CH
        times[off[t] + base:off[t] + base + cnt] += 1
        if tail_twice and cnt % 4:
            times[off[t] + base + 4 * (cnt // 4)] += 1
    return times


# ------------------------------------------------------------------------------------------- SGD

SGD_LATTICE = dict(lr=2.0 ** -3, momentum=0.5, weight_decay=2.0 ** -4)
SGD_TRAIN = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)          # the training configuration's hyper-parameters
# the rounded row, one step; every rounding counted once against the sum of the magnitudes of the terms:
#   buf   the conversions of wd and momentum to fp32, wd p, g + wd p, momentum buf, the add -- 6, terms |g| + |wd p| + |momentum buf0|
#   p     those 6 (scaled by lr), the conversion of lr, lr buf, the subtraction -- 9, terms |p| + lr (|g| + |wd p| + |momentum buf0|)
SGD_N = dict(buf=6, p=9)
SGD_MUTANTS = ["decay_after_momentum", "nesterov", "tail_first_twice", "chunk1_at_8188"]


def _rows_sgd():
    rows = []
    for mom in (0.0, SGD_LATTICE["momentum"]):
        for wd in (0.0, SGD_LATTICE["weight_decay"]):
            for order in ORDERS:
                rows.append(dict(entry="csbsr_sgd_step", kernels=["sgd_step_kernel"], instance=(mom != 0, wd != 0), kind="exact", order=order,
                                 lr=SGD_LATTICE["lr"], momentum=mom, weight_decay=wd, steps=2 if wd else 4))
    rows.append(dict(entry="csbsr_sgd_step", kernels=["sgd_step_kernel"], instance=(True, True), kind="rounded", order="forward", steps=1,
                     n=SGD_N, **SGD_TRAIN))
    rows.append(dict(entry="csbsr_sgd_step", kernels=[], kind="empty"))                                    # nblocks = 0: returns 0, launches nothing
    rows.append(dict(entry="csbsr_sgd_step", kernels=[], kind="refused", momentum=-0.5, weight_decay=0.0))
    rows.append(dict(entry="csbsr_sgd_step", kernels=[], kind="refused", momentum=0.5, weight_decay=-2.0 ** -4))
    return rows


@functools.lru_cache(maxsize=None)
def sgd_inputs(kind, steps):
    """flat float64 p0, buf0 and one g per step over opt_sizes('sgd') (exact: integers in [-64, 64] x 2^-6, a quarter of them zero;
    rounded: normal draws, g with exact zeros)"""
    n = int(sum(opt_sizes("sgd")))
    if kind == "exact":
        return dict(p=lat((n,), 6, 64, (n, 1), 0.75), buf=lat((n,), 6, 64, (n, 2), 0.75), g=[lat((n,), 6, 64, (n, 3 + s), 0.75) for s in range(steps)])
    r = np.random.RandomState(77)
    g = (r.standard_normal(n) * 0.1).astype(f32).astype(np.float64)
    g[r.random_sample(n) < 0.1] = 0.0
    return dict(p=r.standard_normal(n).astype(f32).astype(np.float64), buf=(r.standard_normal(n) * 0.1).astype(f32).astype(np.float64), g=[g])


def sgd_ref(p, buf, gs, lr, momentum, weight_decay, times=None, prove=None, mutant=None):
    """(p, buf, terms) in fp64 after len(gs) steps.  ``times`` (per element): how often each step's update is applied (stepped()).
    ``prove``: a label -- every intermediate is asserted fp32-exact.  terms: (|g| + |wd p| + |mom buf|, |p| + lr x that) of the LAST step,
    for the counted bound.  mutant 'decay_after_momentum': buf = mom buf + g and the update is buf + wd p; 'nesterov': the update is
    d + mom buf"""
    p, b = np.array(p, np.float64), np.array(buf, np.float64)
    times = np.ones(p.shape, np.int64) if times is None else times
    terms = None
    for s, g in enumerate(gs):
        for k in range(int(times.max()) if times.size else 0):
            on = times > k
            wp = weight_decay * p
            d = g + wp if weight_decay != 0 else g
            if momentum != 0:
                mb = momentum * b
                if mutant == "decay_after_momentum":
                    nb = mb + g
                    upd = nb + wp
                else:
                    nb = mb + d
                    upd = d + momentum * nb if mutant == "nesterov" else nb
            else:
                mb, nb, upd = 0.0 * b, b, d
            step = lr * upd
            np_ = p - step
            terms = (np.abs(g) + np.abs(wp) * (weight_decay != 0) + np.abs(mb), np.abs(p) + lr * (np.abs(g) + np.abs(wp) * (weight_decay != 0) + np.abs(mb)))
            if prove:
                for name, v in (("wd p", wp), ("d", d), ("mom buf", mb), ("buf", nb), ("lr buf", step), ("p", np_)):
                    assert_fp32_exact(_t(v), f"{prove} step {s + 1}: {name}")
            p, b = np.where(on, np_, p), np.where(on, nb, b)
    return p, b, terms


def sgd32(p, buf, g, lr, momentum, weight_decay):
    """one step in float32, one rounding per operation, nothing fused (the honest evaluation the counted bound is sized for)"""
    p, b, g = p.astype(f32), buf.astype(f32), g.astype(f32)
    d = g + f32(weight_decay) * p if weight_decay != 0 else g
    if momentum != 0:
        b = f32(momentum) * b + d
        d = b
    return p - f32(lr) * d, b


@functools.lru_cache(maxsize=None)
def sgd_case(kind, momentum, weight_decay, steps, lr):
    """inputs and the reference of one SGD row (shared, read-only), exactness proved for kind == 'exact'"""
    d = dict(sgd_inputs(kind, steps))
    what = f"sgd mom={momentum} wd={weight_decay}"
    d["ref_p"], d["ref_buf"], terms = sgd_ref(d["p"], d["buf"], d["g"], lr, momentum, weight_decay, prove=what if kind == "exact" else None)
    if kind == "rounded":
        d["bound_buf"], d["bound_p"] = SGD_N["buf"] * U * terms[0], SGD_N["p"] * U * terms[1]
    return d


def sgd_row_case(row):
    return sgd_case(row["kind"], row["momentum"], row["weight_decay"], row["steps"], row["lr"])


def sgd_compare(row, got_p, got_buf, what="sgd"):
    """the row's comparison: float32 flat arrays (forward tensor order) against the row's reference; returns {name: error / bound} of
    a rounded row"""
    d = sgd_row_case(row)
    if row["kind"] == "exact":
        check_bits(got_p, d["ref_p"].astype(f32), f"{what}: p")
        if row["momentum"] != 0:
            check_bits(got_buf, d["ref_buf"].astype(f32), f"{what}: buf")
        return {}
    return dict(p=check_bound(got_p, d["ref_p"], d["bound_p"], f"{what}: p"), buf=check_bound(got_buf, d["ref_buf"], d["bound_buf"], f"{what}: buf"))


def sgd_mutant_applies(name, row):
    if row["kind"] not in ("exact", "rounded"):
        return False
    if name == "decay_after_momentum":
        return row["momentum"] != 0 and row["weight_decay"] != 0
    if name == "nesterov":
        return row["momentum"] != 0
    return True


def sgd_mutant(name, row):
    """(p, buf) float32 as a subtly wrong kernel would leave them"""
    d = sgd_row_case(row)
    sizes = opt_sizes("sgd")
    times = None
    if name in ("tail_first_twice", "chunk1_at_8188"):
        idx, bt, bc = block_map(sizes, row["order"])
        times = stepped(sizes, idx, bt, bc, chunk1_base=constants()["CHUNK"] - 4 if name == "chunk1_at_8188" else None, tail_twice=name == "tail_first_twice")
    p, b, _ = sgd_ref(d["p"], d["buf"], d["g"], row["lr"], row["momentum"], row["weight_decay"], times=times,
                      mutant=name if name in ("decay_after_momentum", "nesterov") else None)
    return p.astype(f32), b.astype(f32)


# ------------------------------------------------------------------------------------------- Adam

ADAM_LATTICE = dict(betas=(0.5, 0.75), eps=2.0 ** -10)
ADAM_TRAIN = dict(lr=2e-5, betas=(0.9, 0.999), eps=1e-8)            # the training configuration's hyper-parameters
ADAM_STEPS = 3
ADAM_ROUNDED_T = 3                                                  # the step count the rounded row's bias corrections are taken at
# the rounded row, one step; every rounding counted once:
#   m   the conversion of w1, g - m, the product, the add -- 4, terms |m| + w1 (|g| + |m|)
#   v   the conversions of beta2 and w2, v beta2, w2 g, (w2 g) g, the add -- 6, terms v beta2 + w2 g g (no cancellation: relative)
#   p   m's 4; the denominator, relative (all its terms are positive): v's 6 halved by the root -- 3, the root, the conversion of bc2_sqrt, the
#       division, the conversion of eps, the add -- 8; m / denom; the conversion of step_size and the product; the subtraction -- 4 + 8 + 1 +
#       2 + 1 = 16, terms |p| + step_size (|m| + w1 (|g| + |m|)) / denom
ADAM_N = dict(m=4, v=6, p=16)
ADAM_MUTANTS = ["eps_in_sqrt", "bc2_multiplies", "v_from_new_m", "tail_first_twice", "chunk1_at_8188"]


def adam_table(kind):
    """per tensor (step_size, bc2_sqrt) as Python doubles.  exact: powers of two that differ from tensor to tensor (a row of the table
    read for the wrong tensor shows); rounded: the true bias corrections of step ADAM_ROUNDED_T by the host code's formulas"""
    n = len(opt_sizes("adam"))
    if kind == "exact":
        return [(2.0 ** -(2 + i % 3), 2.0 ** -(i % 2)) for i in range(n)]
    b1, b2 = ADAM_TRAIN["betas"]
    return [host_adam_scalars(ADAM_TRAIN["lr"], b1, b2, ADAM_ROUNDED_T)] * n


def host_adam_scalars(lr, beta1, beta2, t):
    """(step_size, bc2_sqrt) by the Python-double formulas of csbsr_amd/optim.py"""
    import math
    return lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)


def _rows_adam():
    rows = [dict(entry="csbsr_adam_step", kernels=["adam_step_kernel"], kind="exact", order=o, steps=ADAM_STEPS, **ADAM_LATTICE) for o in ORDERS]
    rows.append(dict(entry="csbsr_adam_step", kernels=["adam_step_kernel"], kind="rounded", order="forward", steps=1, n=ADAM_N,
                     betas=ADAM_TRAIN["betas"], eps=ADAM_TRAIN["eps"]))
    rows.append(dict(entry="csbsr_adam_step", kernels=[], kind="empty"))
    return rows


def _exact_product(a, b, what):
    """a b (float32 operands) needs no rounding in fp32 -- proved in fp64, which holds the 48-bit product exactly"""
    r = a.astype(np.float64) * np.float64(b) if np.isscalar(b) else a.astype(np.float64) * b.astype(np.float64)
    assert_fp32_exact(_t(r), what)


def fma32(a, b, c):
    """float32(a b + c) with ONE rounding (a, b, c float32): the product is exact in fp64; the fp64 sum is made round-to-odd from its
    TwoSum residual, after which the rounding to fp32 is the correct rounding of the exact value"""
    pr = a.astype(np.float64) * b.astype(np.float64)
    c = np.asarray(c, np.float64)
    s = pr + c
    bb = s - pr
    err = (pr - (s - bb)) + (c - bb)
    odd = (bits(s) & np.uint64(1)).astype(bool)
    other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    return np.where((err != 0) & ~odd, other, s).astype(f32)


def adam32(p, m, v, gs, step_size, bc2_sqrt, beta1, beta2, eps, times=None, prove=None, mutant=None, fused_update=False):
    """(p, m, v) float32 after len(gs) steps: the kernel's sequence operation by operation, one float32 rounding each.  step_size and
    bc2_sqrt: float32 per element (or per step a list of them).  ``prove``: a label -- the products that feed an add are asserted
    fp32-exact.  fused_update: the last operation as ONE fused multiply-add (what a contracting compiler makes of it; identical
    where step_size is a power of two).  mutants: 'eps_in_sqrt' sqrt(v + eps) / bc2; 'bc2_multiplies' sqrt(v) bc2 + eps;
    'v_from_new_m' (w2 m) m for (w2 g) g"""
    p, m, v = p.astype(f32), m.astype(f32), v.astype(f32)
    w1, b2, w2, e = f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2), f32(eps)
    times = np.ones(p.shape, np.int64) if times is None else times
    for s, g in enumerate(gs):
        g = g.astype(f32)
        ss = (step_size[s] if isinstance(step_size, list) else step_size).astype(f32)
        bc = (bc2_sqrt[s] if isinstance(bc2_sqrt, list) else bc2_sqrt).astype(f32)
        for k in range(int(times.max()) if times.size else 0):
            on = times > k
            gm = g - m
            nm = m + w1 * gm
            src = nm if mutant == "v_from_new_m" else g
            w2g = w2 * src
            nv = v * b2 + w2g * src
            if mutant == "eps_in_sqrt":
                denom = np.sqrt(nv + e) / bc
            elif mutant == "bc2_multiplies":
                denom = np.sqrt(nv) * bc + e
            else:
                denom = np.sqrt(nv) / bc + e
            q = nm / denom
            np_ = fma32(-ss, q, p) if fused_update else p - ss * q
            if prove:
                for name, a, b in (("w1 (g - m)", gm, w1), ("v beta2", v, b2), ("w2 g", src, w2), ("(w2 g) g", w2g, src), ("step_size q", q, ss)):
                    _exact_product(a, b, f"{prove} step {s + 1}: {name}")
            p, m, v = np.where(on, np_, p), np.where(on, nm, m), np.where(on, nv, v)
    return p, m, v


def adam_ref64(p, m, v, g, step_size, bc2_sqrt, beta1, beta2, eps):
    """one step in fp64 with the hyper-parameters as the doubles the host holds; (p, m, v, terms of p)"""
    w1 = 1.0 - beta1
    nm = m + w1 * (g - m)
    nv = v * beta2 + (1.0 - beta2) * g * g
    denom = np.sqrt(nv) / bc2_sqrt + eps
    tm = np.abs(m) + w1 * (np.abs(g) + np.abs(m))
    return p - step_size * (nm / denom), nm, nv, tm, np.abs(p) + step_size * tm / denom


def per_element(values, sizes):
    return np.concatenate([np.full(n, x, np.float64) for x, n in zip(values, sizes)])


@functools.lru_cache(maxsize=None)
def adam_case(kind):
    """inputs and the reference of the Adam rows (shared, read-only), exactness proved for kind == 'exact'.  exact: m = v = 0 at the start,
    as the optimiser creates them; a quarter of g is zero, so that after step 1 v == 0 occurs (denom == eps, m / eps == 0)"""
    sizes = opt_sizes("adam")
    n = int(sum(sizes))
    tab = adam_table(kind)
    d = dict(table=tab, step_size=per_element([t[0] for t in tab], sizes), bc2_sqrt=per_element([t[1] for t in tab], sizes))
    if kind == "exact":
        b1, b2 = ADAM_LATTICE["betas"]
        d.update(p=lat((n,), 6, 64, (n, 11), 0.75), m=np.zeros(n), v=np.zeros(n), g=[lat((n,), 5, 31, (n, 12 + s), 0.75) for s in range(ADAM_STEPS)])
        assert ((d["g"][0] == 0) & (d["g"][1] != 0)).any()
        p, m, v = adam32(d["p"], d["m"], d["v"], d["g"], d["step_size"], d["bc2_sqrt"], b1, b2, ADAM_LATTICE["eps"], prove="adam")
        d.update(ref_p=p, ref_m=m, ref_v=v)
        return d
    r = np.random.RandomState(78)
    g = (r.standard_normal(n) * 0.1).astype(f32).astype(np.float64)
    g[r.random_sample(n) < 0.1] = 0.0
    d.update(p=r.standard_normal(n).astype(f32).astype(np.float64), m=(r.standard_normal(n) * 0.05).astype(f32).astype(np.float64),
             v=((r.standard_normal(n) * 0.1) ** 2).astype(f32).astype(np.float64), g=[g])
    b1, b2 = ADAM_TRAIN["betas"]
    p, m, v, tm, tp = adam_ref64(d["p"], d["m"], d["v"], g, d["step_size"], d["bc2_sqrt"], b1, b2, ADAM_TRAIN["eps"])
    d.update(ref_p=p, ref_m=m, ref_v=v, bound_m=ADAM_N["m"] * U * tm, bound_v=ADAM_N["v"] * U * v, bound_p=ADAM_N["p"] * U * tp)
    return d


def adam_compare(row, got_p, got_m, got_v, what="adam"):
    d = adam_case(row["kind"])
    if row["kind"] == "exact":
        for name, got in (("m", got_m), ("v", got_v), ("p", got_p)):
            check_bits(got, d["ref_" + name], f"{what}: {name}")
        return {}
    return {name: check_bound(got, d["ref_" + name], d["bound_" + name], f"{what}: {name}") for name, got in (("m", got_m), ("v", got_v), ("p", got_p))}


def adam_mutant(name, row):
    d = adam_case(row["kind"])
    sizes = opt_sizes("adam")
    times = None
    if name in ("tail_first_twice", "chunk1_at_8188"):
        idx, bt, bc = block_map(sizes, row["order"])
        times = stepped(sizes, idx, bt, bc, chunk1_base=constants()["CHUNK"] - 4 if name == "chunk1_at_8188" else None, tail_twice=name == "tail_first_twice")
    b1, b2 = row["betas"]
    return adam32(d["p"], d["m"], d["v"], d["g"], d["step_size"].astype(f32), d["bc2_sqrt"].astype(f32), b1, b2, row["eps"], times=times,
                  mutant=name if times is None else None)


# ------------------------------------------------------------------------------------------- the wrappers' runs (optim.SGD / optim.Adam)

WRAP_SIZES = (5, 1028, 8193)          # parameter sizes of the wrapper-level runs; parameter 1 has no gradient in step 2
WRAP_STEPS = 3
WRAP_SGD = dict(lr=2.0 ** -3, momentum=0.5, weight_decay=2.0 ** -4)
WRAP_ADAM = dict(lr=2.0 ** -3, betas=(0.5, 0.75), eps=2.0 ** -10)


def wrap_has_grad(k, step):
    return not (k == 1 and step == 1)


@functools.lru_cache(maxsize=None)
def wrap_case(kind):
    """per parameter the inputs of the three steps and the expected state.  SGD: p and g integers in {-2 .. 2}: three steps with decay stay
    fp32-exact (proved), so the plain fp64 sequence is the one legitimate result.  Adam: the lattice of the exact rows; step_size = lr / (1 -
    beta1^t) is no power of two from t = 2 on, so the LAST operation of a step, p - step_size q, legitimately has two results (fused or
    not) and p is held to the set of sequences {fused, unfused}^steps; m and v have one result each"""
    out = []
    for k, n in enumerate(WRAP_SIZES):
        steps = [s for s in range(WRAP_STEPS) if wrap_has_grad(k, s)]
        if kind == "sgd":
            c = dict(p=lat((n,), 0, 2, (n, 21), 0.8), g=[lat((n,), 0, 2, (n, 22 + s), 0.8) for s in range(WRAP_STEPS)])
            c["ref_p"], c["ref_buf"], _ = sgd_ref(c["p"], np.zeros(n), [c["g"][s] for s in steps], WRAP_SGD["lr"], WRAP_SGD["momentum"],
                                                  WRAP_SGD["weight_decay"], prove=f"optim.SGD parameter {k}")
        else:
            b1, b2 = WRAP_ADAM["betas"]
            c = dict(p=lat((n,), 6, 64, (n, 31), 0.75), g=[lat((n,), 5, 31, (n, 32 + s), 0.75) for s in range(WRAP_STEPS)])
            sc = [host_adam_scalars(WRAP_ADAM["lr"], b1, b2, t + 1) for t in range(len(steps))]          # t counts the parameter's OWN steps
            cands = [c["p"].astype(f32)]
            m = v = np.zeros(n, f32)
            for t, s in enumerate(steps):
                ss, bc = np.full(n, sc[t][0]).astype(f32), np.full(n, sc[t][1]).astype(f32)
                nxt = []
                for fused in (False, True):
                    for p in cands:
                        pp, nm, nv = adam32(p, m, v, [c["g"][s]], ss, bc, b1, b2, WRAP_ADAM["eps"], fused_update=fused)
                        nxt.append(pp)
                cands, m, v = nxt, nm, nv
            c.update(ref_m=m, ref_v=v, ref_p_any=cands, t=len(steps))
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------- head1_fwd

HEAD1_C = (64, 128, 256)
HEAD1_BIAS = 0.375
# sigmoid = 1: out = 1 / (1 + __expf(-t)), t exact.  Relative to sigmoid64(t) (d sigmoid / sigmoid = -(e / (1 + e)) de / e, at most |de / e|):
#   the rounded product (-t) log2(e) inside __expf: 2^-24 |t log2 e| absolute on the exponent, |t| 2^-24 relative on e -- |t|;
#   the hardware exponential v_exp_f32, 1 ulp = 2 x 2^-24 relative -- 2;  the add 1 + e -- 1;  the division -- 1.
HEAD1_T_MAX = 8.0


def head1_sigmoid_n(t):
    return np.abs(t) + 4.0


def head1_ppb(c):
    return constants()["BLOCK"] // (c // 8)


def head1_wrap_npix(c):
    """the smallest pixel count at which the grid-stride loop of head1_fwd_kernel takes a second turn, plus one block and one pixel"""
    return constants()["CAP"] * head1_ppb(c) + head1_ppb(c) + 1


def head1_npix(c):
    p = head1_ppb(c)
    return (1, p - 1, p, p + 1)


def _rows_head1_fwd():
    rows = []
    for c in HEAD1_C:
        k = [f"head1_fwd_kernel<{c // 8}>"]
        for split_ in (0, 1):
            for lay in LAYOUTS:
                for bias in (0, 1):
                    for npix in head1_npix(c):
                        for sg in (0, 1):
                            rows.append(dict(entry="csbsr_head1_fwd", kernels=k, c=c, split=split_, layout=lay, bias=bias, npix=npix, sigmoid=sg, wrap=False))
        for sg in (0, 1):
            rows.append(dict(entry="csbsr_head1_fwd", kernels=k, c=c, split=0, layout="whole", bias=1, npix=head1_wrap_npix(c), sigmoid=sg, wrap=True))
    rows.append(dict(entry="csbsr_head1_fwd", kernels=[], refused="c", c=32, ld=32))
    rows.append(dict(entry="csbsr_head1_fwd", kernels=[], refused="ld", c=64, ld=56))
    return rows


@functools.lru_cache(maxsize=2)
def head1_case(c, npix, split_):
    """hi, lo (float32, fp16-exact), w (float64), and t0 = sum_c (hi + lo) w in fp64, exact in fp32 in any fold order (proved)"""
    key = (c, npix, split_, 41)
    hi = lat32((npix, c), 2, 3, key + (1,), 0.5)
    lo = lat32((npix, c), 8, 7, key + (2,), 0.5) if split_ else None
    w = lat((c,), 4, 7, key + (3,), 0.75)
    w[[0, c - 8, c - 1]] = [2.0 ** -4, -3 * 2.0 ** -4, 5 * 2.0 ** -4]          # the first lane, the last octet and its last element count
    hi[:, c - 1] = np.where(hi[:, c - 1] == 0, 0.25, hi[:, c - 1])
    what = f"head1_fwd c={c} npix={npix} split={split_}"
    x = hi.astype(np.float64) + (lo.astype(np.float64) if split_ else 0.0)
    assert_fp32_exact(_t(x.ravel()[:1 << 20]), what + " hi + lo")          # (2^-8 lattice below 1: nine bits, whichever elements)
    assert np.abs(x).max() <= 0.75 + 7 * 2.0 ** -8
    assert_sum_bound(c + 1, 1.0, 1.0, 2.0 ** -12, what)                      # c products of at most 1 x 1 and the bias, in units of 2^-12
    t0 = x @ w
    del x
    for b in (0.0, HEAD1_BIAS):
        assert_fp32_exact(_t(t0 + b), what)
        assert np.abs(t0 + b).max() <= HEAD1_T_MAX, f"{what}: |t| = {np.abs(t0 + b).max()} > {HEAD1_T_MAX}"
    return dict(hi=hi, lo=lo, w=w, t0=t0)


def sigmoid64(t):
    return 1.0 / (1.0 + np.exp(-np.asarray(t, np.float64)))


def head1_ref(row, t0=None):
    """(reference, bound) of a row: t = t0 + bias and a zero bound, or sigmoid64(t) and its counted bound"""
    t = (head1_case(row["c"], row["npix"], row["split"])["t0"] if t0 is None else t0) + (HEAD1_BIAS if row["bias"] else 0.0)
    if not row["sigmoid"]:
        return t, np.zeros_like(t)
    s = sigmoid64(t)
    return s, head1_sigmoid_n(t) * U * s


def head1_compare(row, got, what="head1_fwd"):
    ref, bound = head1_ref(row)
    if not row["sigmoid"]:
        check_bits(got, ref.astype(f32), what)
        return 0.0
    return check_bound(got, ref, bound, what)


HEAD1_MUTANTS = ["drop_last_octet", "ignore_lo", "wrap_px_minus_grid"]


def head1_mutant_applies(name, row):
    if "refused" in row:
        return False
    return {"drop_last_octet": True, "ignore_lo": bool(row["split"]), "wrap_px_minus_grid": row["wrap"]}[name]


def head1_mutant(name, row):
    """the float32 output of a subtly wrong kernel.  drop_last_octet: channels c - 8 .. c - 1 not summed; ignore_lo: the hi plane alone;
    wrap_px_minus_grid: on its second turn the grid-stride loop reads pixel px - grid (grid = the capped number of workgroups)"""
    d = head1_case(row["c"], row["npix"], row["split"])
    c = row["c"]
    if name == "drop_last_octet":
        x = d["hi"][:, c - 8:].astype(np.float64) + (d["lo"][:, c - 8:] if row["split"] else 0.0)
        t0 = d["t0"] - x @ d["w"][c - 8:]
    elif name == "ignore_lo":
        t0 = d["hi"].astype(np.float64) @ d["w"]
    else:
        first = constants()["CAP"] * head1_ppb(c)
        src = np.arange(row["npix"])
        src[first:] -= constants()["CAP"]
        t0 = d["t0"][src]
    ref, _ = head1_ref(row, t0)
    return ref.astype(f32)


# ------------------------------------------------------------------------------------------- head1_bwd_input

HEAD1B_C = (8, 40, 64, 256)
HEAD1B_WRAP = (256, 65541)          # total = npix c / 8 octets: 2 097 312 > 256 x 8192 = 2 097 152


def _rows_head1_bwd():
    rows = []
    for c in HEAD1B_C:
        for dld in (8, 16):
            for lay in LAYOUTS:
                for npix in (1, 33):
                    for weights in ("lattice", "random"):
                        rows.append(dict(entry="csbsr_head1_bwd_input", kernels=["head1_bwd_input_kernel"], c=c, dpre_ld=dld, layout=lay, npix=npix,
                                         weights=weights, wrap=False))
    for weights in ("lattice", "random"):
        rows.append(dict(entry="csbsr_head1_bwd_input", kernels=["head1_bwd_input_kernel"], c=HEAD1B_WRAP[0], dpre_ld=8, layout="whole",
                         npix=HEAD1B_WRAP[1], weights=weights, wrap=True))
    rows.append(dict(entry="csbsr_head1_bwd_input", kernels=[], refused="c", c=12))
    return rows


@functools.lru_cache(maxsize=2)
def head1b_case(c, npix, weights):
    """d [npix] on 2^-2 {-15 .. 15} (fp16-exact, zeros included), w [c] float32: on 2^-4 {-15 .. 15} or random with 2^-6 <= |w| < 2.  Every
    fp32 product is zero or has 2^-14 <= |d w| < 65504 (asserted): no fp16 subnormal or overflow, the denormal mode is not in question"""
    key = (c, npix, len(weights), 51)
    d = lat32((npix,), 2, 15, key + (1,), 0.8)
    d[-1] = -3.75
    if npix > 1:
        d[0] = 0.0
    if weights == "lattice":
        w = lat32((c,), 4, 15, key + (2,), 0.9)
    else:
        r = np.random.RandomState(c + npix)
        w = (r.uniform(2.0 ** -6, 2.0, c) * r.choice([-1.0, 1.0], c)).astype(f32)
    w[-1] = w[-1] if w[-1] != 0 else f32(0.5)
    prod = d[:, None] * w[None, :]                     # float32 x float32 -> float32: one correctly rounded product
    a = np.abs(prod)
    assert ((a == 0) | ((a >= 2.0 ** -14) & (a < 65504))).all(), f"head1_bwd_input c={c} {weights}: a product in fp16's subnormal or overflow range"
    ref = prod.astype(np.float16)                      # round to nearest even
    if weights == "lattice":
        assert_fp16_exact(_t(d[:, None].astype(np.float64) * w[None, :].astype(np.float64)), f"head1_bwd_input c={c} lattice")
    return dict(d=d, w=w, ref=ref)


def head1b_compare(row, got, what="head1_bwd_input"):
    check_bits(got, head1b_case(row["c"], row["npix"], row["weights"])["ref"], what)


HEAD1B_MUTANTS = ["w_to_fp16_first"]


def head1b_mutant_applies(name, row):
    return "refused" not in row and row["weights"] == "random"          # (a lattice weight IS an fp16 value)


def head1b_mutant(name, row):
    d = head1b_case(row["c"], row["npix"], row["weights"])
    return (d["d"][:, None] * d["w"].astype(np.float16).astype(f32)[None, :]).astype(np.float16)


# ------------------------------------------------------------------------------------------- sigmoid_bwd_to_nhwc8

SIGB_SCALES = (1.0, 2.0 ** -3, 0.3)
# against fp64: dp p, 1 - p and their product -- three fp32 roundings of |ref| -- and 2^-11 |ref| for the fp16 store.  The product with
# the scale is exact for the two powers of two; for 0.3 the reference takes float32(0.3) and the statement as written rounds a fourth
# time (the device does not: sigb_compare) -- 2^-24 against the store's 2^-11; test_step_tail_cases_cpu.py holds the twice-rounded
# restatement to this bound on every row, the 2 097 155-pixel ones included
SIGB_N = 3


def sigb_wrap_npix():
    return constants()["CAP"] * constants()["BLOCK"] + 3


def _rows_sigb():
    return [dict(entry="csbsr_sigmoid_bwd_to_nhwc8", kernels=["sigmoid_bwd_to_nhwc8_kernel"], npix=npix, scale=s, wrap=npix > 257)
            for npix in (1, 255, 257, sigb_wrap_npix()) for s in SIGB_SCALES]


@functools.lru_cache(maxsize=3)
def sigb_case(npix, scale):
    """dp with 2^-3 <= |dp| < 4 and exact zeros, p in [0.05, 0.95] and exactly 0, 1 and 1/2 (float32, otherwise arbitrary): every result
    is zero or an fp16 normal (asserted)"""
    r = np.random.RandomState(npix % 100003 + int(scale * 64))
    dp = (r.uniform(0.125, 4.0, npix) * r.choice([-1.0, 1.0], npix)).astype(f32)
    dp[r.random_sample(npix) < 0.05] = 0.0
    p = r.uniform(0.05, 0.95, npix).astype(f32)
    special = (0.0, 1.0, 0.5)
    if npix >= 6:
        p[[0, 1, 2, npix - 3, npix - 2, npix - 1]] = special + special
        dp[[0, 1, 2, npix - 3, npix - 2, npix - 1]] = [1.5, -2.5, 3.0, -1.5, 2.5, -3.0]
    else:
        p[0], dp[0] = special[SIGB_SCALES.index(scale)], 1.5
    sc = f32(scale)
    v32 = ((dp * p) * (f32(1.0) - p)) * sc
    out = np.zeros((npix, 8), np.float16)
    out[:, 0] = v32.astype(np.float16)
    a = np.abs(v32)
    assert ((a == 0) | ((a >= 2.0 ** -14) & (a < 65504))).all(), f"sigmoid_bwd npix={npix} scale={scale}: a result in fp16's subnormal range"
    v3 = (dp * p) * (f32(1.0) - p)
    once = (v3.astype(np.float64) * np.float64(sc)).astype(np.float16)          # the 48-bit product is exact in fp64: ONE rounding, to fp16
    assert scale == 0.3 or np.array_equal(bits(once), bits(out[:, 0]))         # (a power-of-two scale: nothing to round twice)
    ref64 = dp.astype(np.float64) * p.astype(np.float64) * (1.0 - p.astype(np.float64)) * np.float64(sc)
    return dict(dp=dp, p=p, ref=out, ref_once=once, v32=v32, ref64=ref64, bound=(SIGB_N * U + H16) * np.abs(ref64))


def sigb_compare(row, got, what="sigmoid_bwd_to_nhwc8"):
    """bit for bit against the float32 restatement (all eight channels), and channel 0 against fp64 under the counted bound"""
    d = sigb_case(row["npix"], row["scale"])
    got = np.asarray(got)
    assert got.shape == d["ref"].shape
    check_bits(got[:, 1:], d["ref"][:, 1:], what + " channels 1 .. 7")          # +0.0 bits
    # channel 0: the device folds the LAST two steps, the product with the scale and the fp16 store, into one v_fma_mixlo_f16 (read in
    # the assembly of csrc/image_ops.hip) -- the contraction the optimiser rows are built round, met again where no add is written.  It
    # rounds the exact product ONCE, to fp16, where the statement as written rounds it to fp32 first; at scale 0.3 the two differ in 113
    # of 2 097 155 elements (measured), at a power of two never.  So an element has two legitimate results and must be one of them.
    # Its addend is +0, and (-0) + (+0) is +0: the sign of a ZERO result (IEEE: -0 for dp < 0 at p == 0 or p == 1) is not asked,
    # the convention of the other exact suites.
    g0, twice_, once_ = (a + np.float16(0) for a in (got[:, 0], d["ref"][:, 0], d["ref_once"]))
    bad = (bits(g0) != bits(twice_)) & (bits(g0) != bits(once_))
    if bad.any():
        i = int(np.argmax(bad))
        raise AssertionError(f"{what} channel 0: {int(bad.sum())} of {bad.size} elements are neither rounding, first at {i}: got {g0[i]!r}, "
                             f"want {twice_[i]!r} (or {once_[i]!r})")
    return check_bound(got[:, 0], d["ref64"], d["bound"], what + " against fp64")


SIGB_MUTANTS = ["no_one_minus_p", "writes_channel_1"]


def sigb_mutant_applies(name, row):
    return row["npix"] > 1          # (the one-pixel rows hold p = 0, 1 or 1/2 alone: a zero result hides both)


def sigb_mutant(name, row):
    d = sigb_case(row["npix"], row["scale"])
    out = d["ref"].copy()
    if name == "no_one_minus_p":
        out[:, 0] = ((d["dp"] * d["p"]) * f32(row["scale"])).astype(np.float16)
    else:
        out[:, 1] = out[:, 0]
    return out


# ------------------------------------------------------------------------------------------- coverage

@functools.lru_cache(maxsize=None)
def rows():
    return _rows_sgd() + _rows_adam() + _rows_head1_fwd() + _rows_head1_bwd() + _rows_sigb()


# csrc/multi_tensor.hip: names asserted by another suite (the file that asserts them bit for bit)
COVERED_ELSEWHERE = {
    "csbsr_fingerprint": "test_trainer_dp_gpu.py",
    "fingerprint_kernel": "test_trainer_dp_gpu.py",
}
# csrc/image_ops.hip: every extern "C" entry point without a row here -> the test file that calls it (test_step_tail_cases_cpu.py opens the
# file, and the case modules it imports, and looks for the name)
ELSEWHERE = {
    "csbsr_blur_fwd": "test_image_exact_gpu.py",
    "csbsr_blur_bwd_input": "test_image_exact_gpu.py",
    "csbsr_blur_bwd_kernel": "test_image_exact_gpu.py",
    "csbsr_bicubic_up_add": "test_image_exact_gpu.py",
    "csbsr_aa_bicubic_down_fwd": "test_image_exact_gpu.py",
    "csbsr_aa_bicubic_down_bwd": "test_image_exact_gpu.py",
    "csbsr_area_down_fwd": "test_area_down_gpu.py",
    "csbsr_area_down_bwd": "test_area_down_gpu.py",
    "csbsr_aa_bicubic_up": "test_bicubic_sr_gpu.py",
    "csbsr_bilinear32_fwd": "test_elementwise_exact_gpu.py",
    "csbsr_bilinear32_bwd": "test_elementwise_exact_gpu.py",
    "csbsr_l1_fwd_bwd": "test_metrics_exact_gpu.py",
    "csbsr_segloss_reduce": "test_metrics_exact_gpu.py",
    "csbsr_segloss_finish": "test_metrics_exact_gpu.py",
    "csbsr_sdf": "test_edt_exact_gpu.py",
    "csbsr_crack_weight": "test_crack_weight_gpu.py",
}
NOT_COVERED = {}          # name -> the written reason (six words at least) why it has neither a row nor another suite

_ENTRY = r'extern "C" int (csbsr_\w+)\('
_KERNEL = r"__global__(?: __launch_bounds__\(\d+\))? void (\w+)\("


def source_names(file, text=None):
    """every extern "C" entry point and every __global__ kernel name of csrc/<file>"""
    text = source(file) if text is None else text
    entries, kernels = re.findall(_ENTRY, text), re.findall(_KERNEL, text)
    assert len(kernels) == len(re.findall(r"__global__", text)), f"csrc/{file}: a __global__ line the pattern does not parse"
    assert len(entries) == len(re.findall(r'extern "C"', text)), f'csrc/{file}: an extern "C" line the pattern does not parse'
    return entries, kernels


def _named(table):
    return {r["entry"] for r in table} | {k.split("<")[0] for r in table for k in r["kernels"]}


def missing_names(table=None, elsewhere=None, not_covered=None, text=None):
    """csrc/multi_tensor.hip: the entry points and kernels that no row, no other suite and no written reason accounts for"""
    table = rows() if table is None else table
    elsewhere = COVERED_ELSEWHERE if elsewhere is None else elsewhere
    not_covered = NOT_COVERED if not_covered is None else not_covered
    entries, kernels = source_names("multi_tensor.hip", text)
    named = _named(table)
    return [n for n in entries + kernels if n not in named and n not in elsewhere and n not in not_covered]


def missing_entries(table=None, elsewhere=None, not_covered=None, text=None):
    """csrc/image_ops.hip: the extern "C" entry points that no row, no ELSEWHERE line and no written reason accounts for"""
    table = rows() if table is None else table
    elsewhere = ELSEWHERE if elsewhere is None else elsewhere
    not_covered = NOT_COVERED if not_covered is None else not_covered
    entries, _ = source_names("image_ops.hip", text)
    named = _named(table)
    return [n for n in entries if n not in named and n not in elsewhere and n not in not_covered]


def names_in_test_file(filename):
    """the text of tests/<filename> and of every tests/*_cases.py / abi_harness module it imports"""
    with open(os.path.join(TESTS, filename)) as f:
        text = f.read()
    for mod in re.findall(r"^\s*(?:import|from) (\w+)", text, re.M):
        path = os.path.join(TESTS, mod + ".py")
        if os.path.exists(path):
            with open(path) as f:
                text += f.read()
    return text
