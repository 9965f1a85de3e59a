"""Shared by tests/test_elementwise_cases_cpu.py and tests/test_elementwise_exact_gpu.py: fp64 references, exact-lattice inputs, case
tables, dispatch restatements and reference mutants for the plain-fp16 kernels of csrc/elementwise.hip.  No GPU.

References are the plain definition of each operation in fp64 numpy (every lattice value and every sum of them is an integer multiple
of a power of two far below 2^53, so fp64 holds them exactly):

  class sums      sums[n, k, :] = sum over pixels of onehot(class(y, x) == k) x[n, y, x, :]; border class = (y==0) 8 + (y==H-1) 4 +
                  (x==0) 2 + (x==W-1); ring class = t(y, H) 5 + t(x, W), t = 0, 1, 2, 3, 4 for coordinate 0, 1, interior, size-2, size-1.
  class fill      out[n, y, x, :] = V[n, class(y, x), :] (x (mask > 0 ? 1 : slope)).
  weighted pool   out[n, c] = sum_p w[n, p] x[n, p, c]; dx += w dout; dw = sum_c x dout.
  adaptive pool   the mean over rows [floor(oy H / OH), ceil((oy + 1) H / OH)) x the same in columns, and its adjoint.
  bilinear        two-tap axis matrices M[o, i0] += 1 - w, M[o, i1] += w from the source position of torch's bilinear rule;
                  y = M_y x M_x^T (x the dropout scale of (sample, channel)), dx = M_y^T dy M_x.
  epilogue bwd    d = g act'(pre), pre recovered from the saved output; dres / dres2 by residual mode; dbias = sum_px d;
                  dprelu = sum over pre <= 0 of g pre.
  batch norm      y = drop act((x - mean) invstd gamma + beta + res); backward: dz = dy drop act'(z), red = (sum dz, sum dz xh),
                  dx = gamma invstd (dz - red0 / npix - xh red1 / npix), dgamma += red1, dbeta += red0.

Exactness: every operand is a small integer times a power of two and every builder proves, on the reference, that sums of magnitudes
stay below 2^24 units (any summation order is exact in fp32) and that fp16 results fit 11 significant bits.  Rows that round carry a
counted bound  |got - ref64| <= n 2^-24 sum|terms| (+ 2^-11 |ref64| for an fp16 output), n written next to the row.

Every row is a dict with ``entry`` (the C entry point) and ``kernels`` (the __global__ kernels the call launches, by a restatement of
the host code's gates); missing_names() checks the source's entry points and kernels against them.
"""
import functools
import os
import re

import numpy as np
import torch

from exact_lattice import assert_fp16_exact, assert_fp32_exact, assert_on_lattice, assert_sum_bound, draw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "csbsr_amd", "csrc")
U = 2.0 ** -24          # fp32 unit roundoff
H16 = 2.0 ** -11        # fp16 unit roundoff
MARGIN = 4.0            # an honest fp32 evaluation has to sit this many times inside a counted bound

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_PRELU, ACT_SIGMOID = 0, 1, 2, 3, 4
RES_NONE, RES_ADD, RES_SUB, RES_MUL, RES_FMA = 0, 1, 2, 3, 4

# fp16 maps are tested as a whole map (ld == c) and as channels [8, 8 + c) of a buffer c + 24 channels wide
LAYOUTS = ("whole", "slice")


def layout(name, c):
    """(ld, c0) of a c-channel map in that layout"""
    return (c, 0) if name == "whole" else (c + 24, 8)


# ------------------------------------------------------------------------------------------- what the source states

@functools.lru_cache(maxsize=None)
def source():
    with open(os.path.join(CSRC, "elementwise.hip")) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def constants():
    """the thresholds and tile sizes the tables are built around, read from the lines of csrc/elementwise.hip that state them: a change
    of one of them changes these numbers (or breaks a pattern) and test_elementwise_cases_cpu.py fails the tables"""
    s = source()

    def one(pattern, what):
        m = re.search(pattern, s)
        assert m, f"{what}: pattern {pattern!r} not found in csrc/elementwise.hip"
        return tuple(int(g) for g in m.groups())

    (SEG,) = one(r"constexpr int BCS_SEG = (\d+);", "edge segments")
    (BIG,) = one(r"if \(H >= 3 && W >= 3 && \(long\)H \* W >= (\d+)\) \{", "border_class_sums threshold")
    a, b = one(r"int chunks = \(int\)\(\(hw \+ (\d+)\) / (\d+)\);     // >= 392 workgroups", "border_class_sums chunk rule")
    (BIL_RS,) = one(r"#define BIL_RS (\d+)", "bilinear forward strip")
    (BILB_RS,) = one(r"#define BILB_RS (\d+)", "bilinear backward strip")
    (WP,) = one(r"const int chunks = \(int\)\(\(hw \+ 1023\) / (\d+)\);", "weighted pool chunk")
    e1, e2 = one(r"int blocks = grid_for\(d->npix, ppb \* (\d+), (\d+)\);", "epilogue_bwd grid rule")
    (RPC,) = one(r"const int RPC = (\d+);", "rows per chunk of the partial-row fold")
    assert a == b - 1
    return dict(SEG=SEG, BIG=BIG, CHUNK=b, BIL_RS=BIL_RS, BILB_RS=BILB_RS, WP=WP, EPI_IT=e1, EPI_CAP=e2, RPC=RPC)


def _seed(*key):
    h = 1469598103
    for v in key:
        h = (h * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(h)


def lat(shape, q, amp, key, density=0.5):
    """float64 numpy lattice draw: integers in [-amp, amp] x 2^-q, zero with probability 1 - density"""
    return draw(shape, q, amp, density, _seed(*key)).double().numpy()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def assert_fp16_normal(ref, fp32_bound, what):
    """a bounded fp16 row: below 2^-14 the fp16 store rounds to a multiple of 2^-24, which the 2^-11 |ref| term of the bound does not
    describe -- so no reference value may sit there inexactly unless half the row's fp32 allowance (n 2^-24 sum|terms|) covers the
    2^-25 the store can add (an fp32 evaluation uses at most a quarter of it: MARGIN)"""
    r = np.abs(np.asarray(ref, np.float64))
    half = 0.5 * np.broadcast_to(fp32_bound, r.shape)          # (the store moves a value by at most min(2^-25, |value|))
    bad = (r < 2.0 ** -14) & (_t(r).half().double().numpy() != r) & (np.minimum(2.0 ** -25, r) > half)
    assert not bad.any(), f"{what}: {int(bad.sum())} reference values are fp16-subnormal (smallest {r[bad].min():.3g}): scale the draw"


def _abs_sum_exact(abs_sum, unit, what):
    """sum of magnitudes below 2^24 units: the sum is exact in fp32 in any order (exact_lattice.assert_sum_bound with the magnitudes
    already added up)"""
    assert_sum_bound(1, float(np.max(abs_sum)) if np.size(abs_sum) else 0.0, 1.0, unit, what)


# ------------------------------------------------------------------------------------------- border / ring classes

def border_cls(H, W):
    y, x = np.arange(H)[:, None], np.arange(W)[None, :]
    return (y == 0) * 8 + (y == H - 1) * 4 + (x == 0) * 2 + (x == W - 1) * 1


def ring_t(n, off=0):
    """t = 0, 1, 2, 3, 4 for coordinate 0, 1, interior, n - 2, n - 1 (``off`` = 1: the mutant that takes n - 2 for interior)"""
    i = np.arange(n)
    t = np.full(n, 2)
    t[i >= n - 2 + off] = (i - n + 5)[i >= n - 2 + off]
    t[i < 2] = i[i < 2]
    return t


def ring_cls(H, W, off=0):
    return ring_t(H, off)[:, None] * 5 + ring_t(W, off)[None, :]


def class_sums(x, cls, K, sums0=None):
    """[N, K, c]: one-hot class sums of x [N, H, W, c] (+ sums0)"""
    onehot = (cls[None] == np.arange(K)[:, None, None]).astype(np.float64)
    s = np.einsum("khw,nhwc->nkc", onehot, np.asarray(x, np.float64))
    return s if sums0 is None else s + sums0


def class_fill(V, cls, mask=None, slope=0.0):
    out = np.asarray(V, np.float64)[:, cls, :]          # [N, H, W, c]
    return out if mask is None else out * np.where(np.asarray(mask) > 0, 1.0, slope)


def border_path(H, W):
    return "large" if H >= 3 and W >= 3 and H * W >= constants()["BIG"] else "small"


def border_chunks(hw):
    c = constants()["CHUNK"]
    return min((hw + c - 1) // c, 2048)


SUMS_LARGE = ["bcs_total_kernel", "sum_partials_kernel", "bcs_edges_kernel", "bcs_edges_finish_kernel", "bcs_fixup_kernel"]
SMALL_SHAPES = [(1, 1), (1, 5), (2, 2), (2, 7), (3, 3), (31, 33), (3, 341)]
LARGE_SHAPES = [(3, 342), (4, 256), (32, 32), (23, 45), (70, 66)]
# (N, H, W, c): c = 8 one octet; 24: cpb = 3, ppb = 85, one idle thread; 264: two channel groups in the edge kernels, the second partly
# filled; 2056: c8 = 257 > 256, the cbase loop (one row)
BORDER_SHAPES = [(2, H, W, c) for H, W in SMALL_SHAPES + LARGE_SHAPES for c in (8, 24, 264)] + [(1, 32, 32, 2056)]
RING_SHAPES = [(2, H, W, c) for H, W in [(5, 5), (5, 9), (6, 5), (9, 11), (32, 33), (70, 66)] for c in (8, 24, 264)]
MASK_SLOPE = 0.25


def _rows_border():
    rows = []
    for s in BORDER_SHAPES:
        N, H, W, c = s
        big = border_path(H, W) == "large"
        rows.append(dict(entry="csbsr_border_class_fill", kernels=["border_class_fill_kernel"], shape=s))
        rows.append(dict(entry="csbsr_border_class_fill_masked", kernels=["border_class_fill_kernel"], shape=s))
        rows.append(dict(entry="csbsr_border_class_sums", kernels=SUMS_LARGE if big else ["border_class_sums_small_kernel"], shape=s))
        rows.append(dict(entry="csbsr_border_class_fill_masked_sums", shape=s,
                         kernels=["bcs_fill_total_kernel"] + SUMS_LARGE[1:] if big else ["border_class_fill_kernel", "border_class_sums_small_kernel"]))
        if big:
            rows.append(dict(entry="csbsr_border_class_sums_prelu", kernels=SUMS_LARGE, shape=s))
    for s in RING_SHAPES:
        rows.append(dict(entry="csbsr_ring_class_sums", shape=s,
                         kernels=["bcs_total_kernel", "sum_partials_kernel", "rcs_lines_kernel", "rcs_finish_kernel"]))
    return rows


@functools.lru_cache(maxsize=6)
def class_case(N, H, W, c, ring=False):
    """inputs of one class-sum / class-fill row (float64, lattice values): x in 2^-4 {-15 .. 15} with every pixel within two of the
    edge non-zero (a misplaced border pixel cannot hide); t in 2^-2 {-7 .. 7} with zeros, forced to 0 on half the channels of the two
    pixels either side of every chunk boundary; V distinct per class; mask with exact zeros and negative values; preset sums"""
    K = 25 if ring else 16
    key = (N, H, W, c, K)
    x = lat((N, H, W, c), 4, 15, key + (1,))
    yy, xx = np.arange(H)[:, None], np.arange(W)[None, :]
    near = ((yy < 2) | (yy >= H - 2) | (xx < 2) | (xx >= W - 2))[None, :, :, None]
    x = np.where(near & (x == 0), 2.0 ** -4, x)
    d = dict(x=x, sums0=lat((N, K, c), 4, 2047, key + (2,), density=1.0))
    what = f"class sums {N}x{H}x{W}x{c}"
    assert_sum_bound(H * W + 1, 2047, 1, 1.0, what)          # units of 2^-4: |x| <= 15, |sums0| <= 2047
    if not ring:
        t = lat((N, H, W, c), 2, 7, key + (3,), density=0.7)
        hw, ch = H * W, border_chunks(H * W)
        per = (hw + ch - 1) // ch
        tf = t.reshape(N, hw, c)
        for b in range(per, hw, per):
            tf[:, b - 1:b + 1, ::2] = 0.0
        d["t"] = tf.reshape(N, H, W, c)
        d["negdot0"] = lat((N, c), 6, 2047, key + (4,), density=1.0)
        assert_sum_bound(H * W + 1, 15 * 7, 1, 1.0, what + " negdot")          # units of 2^-6 (the preset: 2047 <= 105 x 20)
        r = lat((N, 16, c), 0, 15, key + (5,), density=1.0)
        d["V"] = (np.arange(16)[None, :, None] * 32 + 16 + r) * 2.0 ** -4 * np.where(np.arange(c) % 2, -1.0, 1.0)      # distinct per class
        d["mask"] = lat((N, H, W, c), 4, 15, key + (6,), density=0.7)
        assert (d["mask"] == 0).any() and (d["mask"] < 0).any()
    return d


@functools.lru_cache(maxsize=16)
def class_reference(kind, N, H, W, c, preset=False):
    """fp64 reference of one row (shared, read-only), bounds proved.  kind: 'sums', 'ring', 'negdot', 'fill', 'fill_masked', 'mask_sums'"""
    d = class_case(N, H, W, c, ring=kind == "ring")
    what = f"{kind} {N}x{H}x{W}x{c}"
    if kind in ("sums", "ring", "mask_sums"):
        src = d["mask"] if kind == "mask_sums" else d["x"]
        r = class_sums(src, ring_cls(H, W) if kind == "ring" else border_cls(H, W), 25 if kind == "ring" else 16, d["sums0"] if preset else None)
        assert_on_lattice(_t(r), 2.0 ** -4, what)
        assert_fp32_exact(_t(r), what)
        return r
    if kind == "negdot":
        r = np.where(d["t"] <= 0, d["x"] * d["t"], 0.0).sum((1, 2)) + (d["negdot0"] if preset else 0.0)
        assert_on_lattice(_t(r), 2.0 ** -6, what)
        assert_fp32_exact(_t(r), what)
        return r
    r = class_fill(d["V"], border_cls(H, W), d["mask"] if kind == "fill_masked" else None, MASK_SLOPE)
    assert_fp16_exact(_t(r), what)
    return r


CLASS_MUTANTS = ["corner_in_edge", "cols_include_corner_rows", "last_segment_dropped", "fixup_subtracts_preset", "ring_typ_off_by_one",
                 "negdot_ungated"]


def class_mutant_applies(name, kind, N, H, W, c, preset):
    if name == "ring_typ_off_by_one":
        return kind == "ring"
    if name == "negdot_ungated":
        return kind == "negdot"
    if kind not in ("sums", "mask_sums"):
        return False
    if name == "last_segment_dropped":
        return border_path(H, W) == "large"
    if name == "fixup_subtracts_preset":
        return border_path(H, W) == "large" and preset
    return True


def class_mutant(name, kind, N, H, W, c, preset):
    """the result a subtly wrong kernel would give.  corner_in_edge: a corner pixel counted into its row's edge class;
    cols_include_corner_rows: the column-edge classes also take the first and last row's pixels of their column; last_segment_dropped:
    the last of the eight segments of every edge line not binned (it stays in the total, so it lands in class 0);
    fixup_subtracts_preset: class 0 = total - the whole content of classes 1 .. 15; ring_typ_off_by_one: coordinate size - 2 taken for
    interior; negdot_ungated: the t > 0 pixels included"""
    d = class_case(N, H, W, c, ring=kind == "ring")
    src = d["mask"] if kind == "mask_sums" else d["x"]
    s0 = d["sums0"] if preset else None
    if name == "ring_typ_off_by_one":
        return class_sums(src, ring_cls(H, W, off=1), 25, s0)
    if name == "negdot_ungated":
        return (d["x"] * d["t"]).sum((1, 2)) + (d["negdot0"] if preset else 0.0)
    cls = border_cls(H, W).copy()
    if name == "corner_in_edge":
        cls[0, :] &= 12
        cls[H - 1, :] &= 12
        return class_sums(src, cls, 16, s0)
    r = class_sums(src, cls, 16, s0)
    if name == "cols_include_corner_rows":
        r[:, 2] += src[:, 0, 0] + (src[:, H - 1, 0] if H > 1 else 0)
        r[:, 1] += src[:, 0, W - 1] + (src[:, H - 1, W - 1] if H > 1 else 0)
        return r
    if name == "last_segment_dropped":
        SEG = constants()["SEG"]
        m = cls.copy()
        m[[0, H - 1], W * (SEG - 1) // SEG:] = 0
        m[1 + (H - 2) * (SEG - 1) // SEG:H - 1, [0, W - 1]] = 0
        return class_sums(src, m, 16, s0)
    assert name == "fixup_subtracts_preset"
    r[:, 0] -= d["sums0"][:, 1:].sum(1)
    return r


# ------------------------------------------------------------------------------------------- weighted pool

WPOOL_SHAPES = [(2, hw, c) for hw in (1, 1023, 1024, 1025, 2100) for c in (8, 64, 320)]          # hw: the 1024-pixel chunk seams


@functools.lru_cache(maxsize=None)
def wpool_case(N, hw, c):
    """x in 2^-4 {-15 .. 15}, w in 2^-6 {-63 .. 63} (pixel 0, the last pixel and the pixels either side of every chunk seam non-zero),
    dout in 2^-4 {-15 .. 15}, dx0 in 2^-4 {-15 .. 15}"""
    key = (N, hw, c, 31)
    d = dict(x=lat((N, hw, c), 4, 15, key + (1,), 0.8), w=lat((N, hw), 6, 63, key + (2,), 0.8), dout=lat((N, c), 4, 15, key + (3,), 0.9),
             dx0=lat((N, hw, c), 4, 15, key + (4,), 0.8))
    WP = constants()["WP"]
    for p in [0, hw - 1] + [q for b in range(WP, hw, WP) for q in (b - 1, b)]:
        d["w"][:, p] = np.where(d["w"][:, p] == 0, 2.0 ** -6, d["w"][:, p])
        d["x"][:, p] = np.where(d["x"][:, p] == 0, 2.0 ** -4, d["x"][:, p])
    what = f"wpool {N}x{hw}x{c}"
    d["out"] = np.einsum("np,npc->nc", d["w"], d["x"])
    _abs_sum_exact(np.einsum("np,npc->nc", np.abs(d["w"]), np.abs(d["x"])), 2.0 ** -10, what)
    d["dw"] = np.einsum("npc,nc->np", d["x"], d["dout"])
    _abs_sum_exact(np.einsum("npc,nc->np", np.abs(d["x"]), np.abs(d["dout"])), 2.0 ** -8, what + " dw")
    d["dx"] = d["dx0"] + d["w"][:, :, None] * d["dout"][:, None, :]
    for k in ("out", "dw"):
        assert_fp32_exact(_t(d[k]), what + " " + k)
    assert_fp16_exact(_t(d["dx"]), what + " dx")
    return d


def wpool_mutant_applies(name, N, hw, c):
    return hw > constants()["WP"]


def wpool_mutant(name, N, hw, c):
    """seam_twice: the first pixel of every chunk but the first counted twice"""
    assert name == "seam_twice"
    d, WP = wpool_case(N, hw, c), constants()["WP"]
    r = d["out"].copy()
    for b in range(WP, hw, WP):
        r += d["w"][:, b, None] * d["x"][:, b]
    return r


WPOOL_MUTANTS = ["seam_twice"]


def _rows_wpool():
    return ([dict(entry="csbsr_weighted_pool_fwd", kernels=["wpool_fwd_kernel", "sum_partials_kernel"], shape=s) for s in WPOOL_SHAPES]
            + [dict(entry="csbsr_weighted_pool_bwd", kernels=["wpool_bwd_kernel"], shape=s) for s in WPOOL_SHAPES])


# ------------------------------------------------------------------------------------------- adaptive average pool

# (N, H, W, OH, OW, c)
AAP_EXACT = [(2, H, W, o, o, c) for H, W, o in [(8, 8, 1), (16, 16, 2), (8, 8, 2), (8, 8, 4), (16, 16, 8)] for c in (8, 24, 136)]
AAP_RAGGED = [(2, H, W, oh, ow, c) for H, W, oh, ow in [(11, 14, 3, 5), (17, 19, 2, 2), (8, 8, 3, 3), (8, 8, 6, 6)] for c in (8, 24, 136)]
# every rounding of the backward's sequence for one input pixel: at most four windows hold it (they overlap by one row / column), each
# costs 1 / count, g x it and the add into the sum (3 x 4), and one more for the add onto dx0; each is at most 2^-24 of sum|terms|
AAP_BWD_ROUNDINGS = 13


def aap_windows(n, o, end_off=0):
    return [(i * n // o, min(-((-(i + 1) * n) // o) + end_off, n)) for i in range(o)]


def aap_kernel_for(H, W, OH, OW):
    return "aap_fwd_block_kernel" if (H // OH) * (W // OW) >= 64 else "aap_fwd_kernel"


def aap_fwd_roundings(count):
    """count - 1 additions (the block kernel: at most count / 32 + 32, fewer), the reciprocal of the count (the block kernel: none), the
    product (the block kernel: the division)"""
    return count + 1


def aap_ref(x, OH, OW, end_off=0):
    """[N, OH, OW, c] window means, and per output the sum of magnitudes / count and the window's pixel count"""
    N, H, W, c = x.shape
    y, ab, cnt = np.zeros((N, OH, OW, c)), np.zeros((N, OH, OW, c)), np.zeros((OH, OW), int)
    for oy, (y0, y1) in enumerate(aap_windows(H, OH, end_off)):
        for ox, (x0, x1) in enumerate(aap_windows(W, OW, end_off)):
            win = x[:, y0:y1, x0:x1]
            cnt[oy, ox] = (y1 - y0) * (x1 - x0)
            y[:, oy, ox] = win.sum((1, 2)) / cnt[oy, ox]
            ab[:, oy, ox] = np.abs(win).sum((1, 2)) / cnt[oy, ox]
    return y, ab, cnt


def aap_bwd_ref(dy, H, W, end_off=0):
    N, OH, OW, c = dy.shape
    dx, ab = np.zeros((N, H, W, c)), np.zeros((N, H, W, c))
    for oy, (y0, y1) in enumerate(aap_windows(H, OH, end_off)):
        for ox, (x0, x1) in enumerate(aap_windows(W, OW, end_off)):
            k = (y1 - y0) * (x1 - x0)
            dx[:, y0:y1, x0:x1] += dy[:, oy, ox][:, None, None] / k
            ab[:, y0:y1, x0:x1] += np.abs(dy[:, oy, ox])[:, None, None] / k
    return dx, ab


@functools.lru_cache(maxsize=None)
def aap_case(N, H, W, OH, OW, c):
    key = (N, H, W, OH, OW, c, 41)
    d = dict(x=lat((N, H, W, c), 4, 15, key + (1,), 0.9), dy=lat((N, OH, OW, c), 4, 15, key + (2,), 0.9), dx0=lat((N, H, W, c), 4, 15, key + (3,), 0.9))
    d["y"], d["y_abs"], d["cnt"] = aap_ref(d["x"], OH, OW)
    d["dx"], d["dx_abs"] = aap_bwd_ref(d["dy"], H, W)
    d["exact"] = bool(all(k & (k - 1) == 0 for k in d["cnt"].ravel()))
    what = f"aap {N}x{H}x{W}->{OH}x{OW} c{c}"
    if d["exact"]:
        assert_sum_bound(int(d["cnt"].max()), 15, 1, 1.0, what)
        assert_fp16_exact(_t(d["y"]), what)
        assert_fp16_exact(_t(d["dx"]), what + " dx")
        assert_fp16_exact(_t(d["dx"] + d["dx0"]), what + " dx accumulated")
    else:
        assert_fp16_normal(d["y"], aap_fwd_roundings(d["cnt"])[None, :, :, None] * U * d["y_abs"], what + " y")
        assert_fp16_normal(d["dx"], AAP_BWD_ROUNDINGS * U * d["dx_abs"], what + " dx")
        assert_fp16_normal(d["dx"] + d["dx0"], AAP_BWD_ROUNDINGS * U * (d["dx_abs"] + np.abs(d["dx0"])), what + " dx accumulated")
    return d


AAP_MUTANTS = ["window_end"]


def aap_mutant_applies(name, N, H, W, OH, OW, c):
    return OH > 1 or OW > 1


def aap_mutant(name, direction, N, H, W, OH, OW, c):
    """window_end: every window ends one row / column late (clipped to the image)"""
    d = aap_case(N, H, W, OH, OW, c)
    return aap_ref(d["x"], OH, OW, end_off=1)[0] if direction == "fwd" else aap_bwd_ref(d["dy"], H, W, end_off=1)[0]


def _rows_aap():
    rows = []
    for s in AAP_EXACT + AAP_RAGGED:
        rows.append(dict(entry="csbsr_adaptive_avgpool_fwd", kernels=[aap_kernel_for(*s[1:5])], shape=s))
        rows.append(dict(entry="csbsr_adaptive_avgpool_bwd", kernels=["aap_bwd_kernel"], shape=s))
    return rows


# ------------------------------------------------------------------------------------------- bilinear resize

def bil_matrix(n_in, n_out, align, half_pixel=True, drop_last=False):
    """fp64 [n_out, n_in]: two taps per output at the source position of torch's rule (align_corners False: (o + .5) in / out - .5
    clamped at 0; True: o (in - 1) / (out - 1)); i0 = floor, i1 = min(i0 + 1, in - 1).  half_pixel / drop_last exist for the mutants"""
    M = np.zeros((n_out, n_in))
    for o in range(n_out):
        if align:
            src = o * (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
        else:
            src = max((o + 0.5) * (n_in / n_out) - 0.5, 0.0) if half_pixel else o * (n_in / n_out)
        i0 = min(int(src), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        M[o, i0] += 1.0 - (src - i0)
        M[o, i1] += src - i0
    if drop_last:
        for i in range(n_in):
            nz = np.nonzero(M[:, i])[0]
            if len(nz):
                M[nz[-1], i] = 0.0
    return M


def bil_apply(My, x, Mx):
    """M_y x M_x^T over the two image axes of x [N, H, W, c] (the adjoint: pass the transposes)"""
    return np.einsum("pw,nowc->nopc", Mx, np.einsum("oh,nhwc->nowc", My, x))


def bilinear_kernel_for(direction, N, H, W, OH, OW, c):
    """the kernel(s) csbsr_bilinear_fwd / _bwd launch: a TRANSCRIPTION of the two gates of csrc/elementwise.hip (the A/B hook at its
    default, a reduction scratch registered)"""
    k, c8 = constants(), c // 8
    if direction == "fwd":
        strips = N * ((OH + k["BIL_RS"] - 1) // k["BIL_RS"])
        cols = OH >= k["BIL_RS"] and strips <= 65535 and (OW * c8 + 255) // 256 * strips >= 64
        return ["bilinear_fwd_cols_kernel" if cols else "bilinear_fwd_kernel"]
    if (OH // H) * (OW // W) >= 64:
        return ["bilinear_bwd_block_kernel"]
    strips = N * ((H + k["BILB_RS"] - 1) // k["BILB_RS"])
    if OH >= H and OW >= W and 2 * OH <= 5 * H and 2 * OW <= 5 * W and strips <= 65535 and (W * c8 + 255) // 256 * strips >= 64:
        return ["bil_tab_kernel", "bilinear_bwd_cols_kernel"]
    return ["bilinear_bwd_kernel"]


# (N, H, W, OH, OW, align_corners, c): dyadic source positions only (x2, x4, x8 at align_corners = 0; (H - 1) | (OH - 1) 2^k at 1)
BIL_EXACT = [
    (2, 5, 7, 10, 14, 0, 8),            # x2: row-major forward, scanning backward
    (2, 5, 7, 20, 28, 0, 24),           # x4, three octets
    (2, 5, 9, 9, 33, 1, 8),             # align_corners: 5 -> 9 and 9 -> 33
    (2, 1, 1, 8, 8, 0, 8),              # one input pixel: the block backward (ratio 64), every tap clamped
    (2, 4, 4, 32, 32, 0, 8),            # x8: the block backward with edges and an interior
    (2, 4, 4, 32, 32, 0, 72),           # ... two channel groups of the block backward, the second one octet wide
    (2, 250, 5, 500, 10, 0, 8),         # 64 strips: the column kernels both ways, the last strip ragged (250 = 31 x 8 + 2, 500 = 31 x 16 + 4)
    (2, 250, 5, 500, 10, 0, 24),
    (2, 129, 33, 257, 65, 1, 64),       # the column kernels with align_corners (source positions o / 2), three column blocks, the last partly filled
]
BIL_KERNELS = ["bilinear_fwd_kernel", "bilinear_fwd_cols_kernel", "bilinear_bwd_kernel", "bilinear_bwd_block_kernel", "bil_tab_kernel",
               "bilinear_bwd_cols_kernel"]
DROP_SCALES = (0.0, 0.5, 1.0, 2.0)


@functools.lru_cache(maxsize=4)
def bilinear_case(N, H, W, OH, OW, align, c):
    """x integers in {-7 .. 7}; dy integers in {-7 .. 7} up to x2, ternary (sparser as the ratio grows) beyond; dx0 integers in {-7 .. 7} (ternary at x8);
    drop: per (sample, channel) scales in {0, .5, 1, 2}, the samples' rows different.  The weights are multiples of 1 / 16 per axis, so
    every product and sum is on 2^-8 and far below 2^24 units; the fp16 stores are proved on the references"""
    key = (N, H, W, OH, OW, align, c, 51)
    ratio = (OH // H) * (OW // W)
    My, Mx = bil_matrix(H, OH, align), bil_matrix(W, OW, align)
    d = dict(My=My, Mx=Mx, x=lat((N, H, W, c), 0, 7, key + (1,), 0.9), dx0=lat((N, H, W, c), 0, 7 if ratio <= 16 else 1, key + (3,), 0.9),
             dy=lat((N, OH, OW, c), 0, 7 if ratio <= 4 else 1, key + (2,), 0.9 if ratio <= 4 else (0.5 if ratio <= 16 else (0.25 if H * W == 1 else 0.1))))
    g = _seed(*key, 4)
    d["drop"] = np.array(DROP_SCALES)[torch.randint(0, 4, (N, c), generator=g).numpy()]
    d["drop"][:2, :4] = [[2.0, 0.0, 0.5, 1.0], [0.5, 1.0, 2.0, 0.0]]          # the two samples' rows differ, every scale occurs
    what = f"bilinear {N}x{H}x{W}->{OH}x{OW} align={align} c{c}"
    for M in (My, Mx):
        assert_on_lattice(_t(M), 2.0 ** -4, what + " weights")
    d["y"], d["dx"] = bil_apply(My, d["x"], Mx), bil_apply(My.T, d["dy"], Mx.T)
    assert_sum_bound(int((My != 0).sum(0).max() * (Mx != 0).sum(0).max()) + 1, 7, 2.0 ** 8, 1.0, what)          # units of 2^-8, any order
    for dr, tag in ((None, ""), (d["drop"][:, None, None, :], " drop")):
        y, dx = (d["y"], d["dx"]) if dr is None else (d["y"] * dr, d["dx"] * dr)
        assert_fp16_exact(_t(y), what + tag)
        assert_fp16_exact(_t(dx), what + " dx" + tag)
        assert_fp16_exact(_t(dx + d["dx0"]), what + " dx accumulated" + tag)
    return d


BIL_MUTANTS = ["no_half_pixel", "bwd_misses_last", "drop_wrong_sample"]


def bilinear_mutant_applies(name, direction, drop, N, H, W, OH, OW, align, c):
    if name == "no_half_pixel":
        return not align and (H > 1 or W > 1)
    if name == "bwd_misses_last":
        return direction == "bwd"
    return bool(drop)


def bilinear_mutant(name, direction, drop, N, H, W, OH, OW, align, c):
    """no_half_pixel: source position o in / out; bwd_misses_last: per input column the last output that references it is not summed;
    drop_wrong_sample: the scale row of the next sample"""
    d = bilinear_case(N, H, W, OH, OW, align, c)
    My, Mx = d["My"], d["Mx"]
    if name == "no_half_pixel":
        My, Mx = bil_matrix(H, OH, 0, half_pixel=False), bil_matrix(W, OW, 0, half_pixel=False)
    if name == "bwd_misses_last":
        Mx = bil_matrix(W, OW, align, drop_last=True)
    dr = d["drop"] if drop else np.ones_like(d["drop"])
    if name == "drop_wrong_sample":
        dr = np.roll(dr, 1, 0)
    r = bil_apply(My, d["x"], Mx) if direction == "fwd" else bil_apply(My.T, d["dy"], Mx.T)
    return r * dr[:, None, None, :]


def _rows_bilinear():
    rows = []
    for s in BIL_EXACT:
        N, H, W, OH, OW, al, c = s
        rows.append(dict(entry="csbsr_bilinear_fwd", kernels=bilinear_kernel_for("fwd", N, H, W, OH, OW, c), shape=s))
        rows.append(dict(entry="csbsr_bilinear_bwd", kernels=bilinear_kernel_for("bwd", N, H, W, OH, OW, c), shape=s))
    return rows


# ------------------------------------------------------------------------------------------- epilogue backward

EPI_SLOPE = {ACT_NONE: 0.0, ACT_RELU: 0.0, ACT_LRELU: 2.0 ** -3, ACT_PRELU: 2.0 ** -2, ACT_SIGMOID: 0.0}
# (npix, c): one block; c8 = 3 (ppb = 85, an idle thread); several blocks at one octet; c = 264 (c8 = 33, ppb = 7, 25 idle threads)
EPI_SHAPES = [(37, 8), (100, 24), (4100, 8), (300, 264)]
# (act, res_mode, dres, dres2): dres / dres2 0 absent, 1 stored, 2 accumulated
EPI_CONFIGS = [(a, r, (i + j) % 3 if r else 0, (1 + (i % 2)) if r == RES_FMA else 0)
               for i, a in enumerate((ACT_NONE, ACT_RELU, ACT_LRELU, ACT_PRELU)) for j, r in enumerate((RES_NONE, RES_ADD, RES_SUB, RES_FMA))]
EPI_CONFIGS += [(ACT_RELU, RES_ADD, 2, 0), (ACT_PRELU, RES_ADD, 1, 0), (ACT_NONE, RES_ADD, 2, 0), (ACT_LRELU, RES_FMA, 2, 2)]
EPI_CONFIGS += [(ACT_SIGMOID, RES_NONE, 0, 0), (ACT_SIGMOID, RES_ADD, 1, 0)]
# ACT_SIGMOID: d = (g y) (1 - y) from the saved output y: 1 - y, g y and their product -- three roundings of |g y (1 - y)|, and the fp16 store
EPI_SIGMOID_ROUNDINGS = 3


# the fold of more than 1024 partial rows takes two levels (csbsr_sum_partials_batched); a block covers 8 ppb pixels of all channels, so the
# smallest such row has 1025 x 8 pixels at ppb = 1: c8 = 129 octets (256 / 129 = 1), ReLU, dbias alone
EPI_FOLD2 = (8200, 1032, ACT_RELU, RES_NONE, 0, 0)


def epi_blocks(npix, c):
    k = constants()
    ppb = 256 // min(c // 8, 256)
    return ppb, min(max((npix + ppb * k["EPI_IT"] - 1) // (ppb * k["EPI_IT"]), 1), k["EPI_CAP"])


@functools.lru_cache(maxsize=8)
def epi_case(npix, c, act, res_mode, dres, dres2):
    """pre in 2^-2 {-3 .. 3} with exact zeros, slope a power of two, res / res2 in 2^-1 {-3 .. 3}, g in 2^-2 {-3 .. 3}, previous
    dres / dres2 in 2^-2 {-7 .. 7}: the saved output out = act(pre) (+ res | - res | + res res2) is fp16-exact and the kernel recovers
    act(pre) from it exactly.  The derivative at pre == 0 is the one torch's relu / leaky_relu / prelu backward use: the NEGATIVE side
    (0 for ReLU, the slope otherwise) -- their test is ``> 0`` -- and the slope gradient takes pre == 0 as the negative side too."""
    key = (npix, c, act, res_mode, dres, dres2, 61)
    slope = EPI_SLOPE[act]
    pre = lat((npix, c), 2, 3, key + (1,), 0.7)
    assert (pre == 0).any()
    yv = pre if act == ACT_NONE else np.where(pre > 0, pre, pre * slope)
    if act == ACT_SIGMOID:          # the saved output IS the sigmoid: any fp16 value in (0, 1), here 2^-6 {1 .. 63}
        yv = (torch.randint(1, 64, (npix, c), generator=_seed(*key, 9)).double() * 2.0 ** -6).numpy()
    d = dict(g=lat((npix, c), 2, 3, key + (2,), 0.8), slope=slope, pre=pre, yv=yv,
             dbias0=lat((c,), 2, 15, key + (7,), 1.0), dprelu0=lat((1,), 2, 15, key + (8,), 1.0))
    if res_mode:          # (drawn only where a row reads them: the two-level-fold row is 8.5 million elements per map)
        d.update(res=lat((npix, c), 1, 3, key + (3,), 0.8), res2=lat((npix, c), 1, 3, key + (4,), 0.8),
                 dres0=lat((npix, c), 2, 7, key + (5,), 0.8), dres20=lat((npix, c), 2, 7, key + (6,), 0.8))
    d["out"] = yv + (0.0 if not res_mode else {RES_ADD: d["res"], RES_SUB: -d["res"], RES_FMA: d["res"] * d["res2"]}[res_mode])
    return d


def epi_ref(npix, c, act, res_mode, dres, dres2, relu_at_zero=0.0, drop_last_partial=False, sigmoid_linear=False):
    """dict(dpre, dres, dres2, dbias, dprelu) in fp64, bounds proved; dbias and dprelu are ACCUMULATED onto lattice presets (the fold adds
    into them); ACT_SIGMOID adds dpre_abs, the terms of its bound.  The keyword arguments exist for the mutants"""
    d = epi_case(npix, c, act, res_mode, dres, dres2)
    g, pre, slope = d["g"], d["pre"], d["slope"]
    if act == ACT_NONE:
        dp = g.copy()
    elif act == ACT_RELU:
        dp = np.where(pre > 0, g, np.where(pre == 0, g * relu_at_zero, 0.0))
    elif act == ACT_SIGMOID:
        dp = g * d["yv"] if sigmoid_linear else g * d["yv"] * (1.0 - d["yv"])
    else:
        dp = np.where(pre > 0, g, g * slope)
    r = dict(dpre=dp)
    gr = None if not res_mode else {RES_ADD: g, RES_SUB: -g, RES_FMA: g * d["res2"]}[res_mode]
    if dres:
        r["dres"] = gr + (d["dres0"] if dres == 2 else 0.0)
    if dres2:
        r["dres2"] = g * d["res"] + (d["dres20"] if dres2 == 2 else 0.0)
    contrib = dp
    if drop_last_partial:
        ppb, blocks = epi_blocks(npix, c)
        contrib = np.where(((np.arange(npix) // ppb) % blocks == blocks - 1)[:, None], 0.0, dp)
    r["dbias"] = contrib.sum(0) + d["dbias0"]
    what = f"epilogue_bwd {npix}x{c} act={act} res={res_mode}"
    _abs_sum_exact(np.abs(dp).sum(0) + 4.0, 2.0 ** -14 if act == ACT_SIGMOID else 2.0 ** -5, what + " dbias")
    if act == ACT_PRELU:
        r["dprelu"] = np.where(pre > 0, 0.0, g * pre).sum(keepdims=True).reshape(1) + d["dprelu0"]
        _abs_sum_exact(np.abs(g * pre).sum() + 4.0, 2.0 ** -4, what + " dprelu")
    for k, v in r.items():
        if act == ACT_SIGMOID and k == "dpre":          # g y (1 - y) is exact in fp32 (14 bits) but not in fp16: the store rounds
            assert_fp32_exact(_t(v), what + " dpre before the store")
            assert_fp16_normal(v, EPI_SIGMOID_ROUNDINGS * U * np.abs(v), what + " dpre")
            continue
        (assert_fp32_exact if k in ("dbias", "dprelu") else assert_fp16_exact)(_t(v), what + " " + k)
    if act == ACT_SIGMOID:
        r["dpre_abs"] = np.abs(dp)
    return r


EPI_MUTANTS = ["relu_one_at_zero", "dbias_last_partial", "sigmoid_linear"]


def epi_mutant_applies(name, npix, c, act, res_mode, dres, dres2):
    if name == "sigmoid_linear":
        return act == ACT_SIGMOID
    return act == ACT_RELU if name == "relu_one_at_zero" else epi_blocks(npix, c)[1] > 1


def epi_mutant(name, *row):
    """relu_one_at_zero: a ReLU derivative of 1 at exactly 0; dbias_last_partial: the last partial row not folded; sigmoid_linear: g y
    for g y (1 - y)"""
    if name == "sigmoid_linear":
        return epi_ref(*row, sigmoid_linear=True)
    return epi_ref(*row, relu_at_zero=1.0) if name == "relu_one_at_zero" else epi_ref(*row, drop_last_partial=True)


def _rows_epilogue():
    return [dict(entry="csbsr_epilogue_backward", kernels=["epilogue_bwd_kernel", "sum_partials_kernel"], shape=s)
            for s in [s + cfg for s in EPI_SHAPES for cfg in EPI_CONFIGS] + [EPI_FOLD2]]


# ------------------------------------------------------------------------------------------- small kernels

AXPBY = [(npix, c, a, b, z) for npix, c in [(1, 8), (37, 24), (300, 264)] for a, b, z in [(1.0, 1.0, 1), (0.5, -2.0, 1), (-0.25, 0.0, 0), (2.0, 0.5, 1)]]
SUM_ACT = [(npix, c, n, relu) for npix, c in [(1, 8), (37, 24), (300, 264)] for n in (1, 2, 3, 4) for relu in (0, 1)]
FILL = [(npix, c, v) for npix, c in [(1, 8), (37, 24), (300, 264)] for v in (0.0, -0.375, 1536.0)]
TO_NCHW = [(2, C, 5, 7, a, b) for C in (1, 3, 8) for a, b in [(1.0, 0.0), (1.0, 1.0), (0.5, 1.0), (1.0, 0.5), (0.5, 0.5)]]
TO_NHWC = [(2, C, 5, 7, cp, norm) for C, cp in [(1, 8), (3, 8), (8, 8), (3, 16)] for norm in (0, 1)]
# (N, cout, cin, c0, c1): one and two mean segments; cout = 5: the second block holds one output; 32: eight full blocks
DC_BIAS = [(2, cout, cin, c0, c1) for cout in (5, 32) for cin, c0, c1 in [(24, 24, 0), (70, 40, 30), (200, 130, 70)]]


@functools.lru_cache(maxsize=None)
def small_case(kind, *row):
    """inputs and the fp64 reference of one small-kernel row, bounds proved"""
    key = tuple(int(abs(v) * 16) for v in row) + (len(kind), 71)
    if kind == "axpby":
        npix, c, a, b, z = row
        d = dict(x=lat((npix, c), 4, 15, key + (1,), 0.9), z=lat((npix, c), 4, 15, key + (2,), 0.9))
        d["ref"] = a * d["x"] + (b * d["z"] if z else 0.0)
    elif kind == "sum_act":
        npix, c, n, relu = row
        d = dict(xs=[lat((npix, c), 4, 15, key + (i,), 0.9) for i in range(n)])
        s = sum(d["xs"])
        d["ref"] = np.maximum(s, 0.0) if relu else s
    elif kind == "to_nchw":
        N, C, H, W, a, b = row
        d = dict(src=lat((N, H, W, 8), 4, 15, key + (1,), 0.9), dst0=lat((N, C, H, W), 4, 15, key + (2,), 0.9))
        d["ref"] = b * d["dst0"] + a * d["src"][..., :C].transpose(0, 3, 1, 2)
    elif kind == "to_nhwc":
        N, C, H, W, cp, norm = row
        d = dict(src=lat((N, C, H, W), 4, 15, key + (1,), 0.9), mean=lat((N, C), 4, 15, key + (2,), 1.0),
                 invstd=2.0 ** torch.randint(-2, 3, (N, C), generator=_seed(*key, 3)).double().numpy())
        v = (d["src"] - d["mean"][:, :, None, None]) * d["invstd"][:, :, None, None] if norm else d["src"]
        d["ref"] = np.zeros((N, H, W, cp))
        d["ref"][..., :C] = v.transpose(0, 2, 3, 1)
    else:
        assert kind == "dc_bias"
        N, cout, cin, c0, c1 = row
        d = dict(S=lat((cout, cin), 6, 15, key + (1,), 0.9), m0=lat((N, c0 + 3), 4, 15, key + (2,), 0.9),
                 m1=lat((N, max(c1, 1) + 5), 4, 15, key + (3,), 0.9),
                 bias=lat((cout,), 4, 15, key + (4,), 1.0))
        mm = np.concatenate([d["m0"][:, :c0], d["m1"][:, :c1]], 1)
        d["ref_nobias"] = np.einsum("oc,nc->no", d["S"][:, :c0 + c1], mm)
        d["ref"] = d["ref_nobias"] + d["bias"][None]
        _abs_sum_exact(np.einsum("oc,nc->no", np.abs(d["S"][:, :c0 + c1]), np.abs(mm)) + 15 * 64, 2.0 ** -10, f"dc_bias {row}")
        assert_fp32_exact(_t(d["ref"]), f"dc_bias {row}")
        return d
    what = f"{kind} {row}"
    (assert_fp32_exact if kind == "to_nchw" else assert_fp16_exact)(_t(d["ref"]), what)
    return d


def _rows_small():
    rows = [dict(entry="csbsr_axpby", kernels=["axpby_kernel"], shape=s) for s in AXPBY]
    rows += [dict(entry="csbsr_sum_act", kernels=["sum_act_kernel"], shape=s) for s in SUM_ACT]
    rows += [dict(entry="csbsr_fill_f16", kernels=["fill16_kernel"], shape=s) for s in FILL]
    rows += [dict(entry="csbsr_nhwc16_to_nchw32", kernels=["nhwc16_to_nchw32_kernel"], shape=s) for s in TO_NCHW]
    rows += [dict(entry="csbsr_nchw32_to_nhwc16", kernels=["nchw32_to_nhwc16_kernel"], shape=s) for s in TO_NHWC]
    rows += [dict(entry="csbsr_dc_bias", kernels=["dc_bias_kernel"], shape=s) for s in DC_BIAS]
    return rows


# ------------------------------------------------------------------------------------------- batch norm, plain path

# (N, hw, c): npix = N hw a power of two; c = 8: one reduce block (64 pixels) and two (4096 > 256 x 8); c = 40 (c8 = 5, ppb = 51, one
# idle thread; the grid of the elementwise kernels a multiple of 5): one block (64) and three (1024 > 2 x 408)
BN_SHAPES = [(2, 32, 8), (2, 2048, 8), (2, 32, 40), (2, 512, 40)]
# (act, res, drop, dres): dres 0 absent, 1 stored, 2 accumulated
BN_CONFIGS = [(a, r, dr, ds) for a in (ACT_NONE, ACT_RELU, ACT_PRELU) for r, dr, ds in [(0, 0, 0), (1, 1, 1), (1, 0, 2), (0, 1, 0)]]
BN_SLOPE = 0.25
# dx = (gamma invstd) (dz - red0 / npix - xh red1 / npix): the two scalings by 1 / npix, dz - k1, xh k2, the subtraction, gamma invstd
# and the final product -- seven roundings, each at most 2^-24 of (|gamma invstd| (|dz| + |k1| + |xh k2|)); the sums in red are exact
BN_DX_ROUNDINGS = 7


def bn_blocks(npix, c):
    ppb = 256 // min(c // 8, 256)
    return min(max((npix + ppb * 8 - 1) // (ppb * 8), 1), 1024)


@functools.lru_cache(maxsize=None)
def bn_case(N, hw, c, act, res, drop, dres):
    """x, mean on 2^-4 {-15 .. 15}, invstd in {1/2, 1, 2}, gamma, beta, res on 2^-2 {-3 .. 3}, dy on 2^4 {-3 .. 3} (large enough that no
    dx lands in fp16's subnormal range), dropout scales
    {0, 1/2, 1, 2} per (sample, channel): every product of the forward and every sum of the backward is exact (proved below); the
    reference is the BatchNorm backward formula with the statistics as given"""
    key = (N, hw, c, act, res, drop, dres, 81)
    npix = N * hw
    assert npix & (npix - 1) == 0
    d = dict(x=lat((npix, c), 4, 15, key + (1,), 0.9), mean=lat((c,), 4, 15, key + (2,), 0.9), gamma=lat((c,), 2, 3, key + (3,), 1.0),
             beta=lat((c,), 2, 3, key + (4,), 0.9), res=lat((npix, c), 2, 3, key + (5,), 0.8), dy=lat((npix, c), 2, 3, key + (6,), 0.8) * 64,
             dres0=lat((npix, c), 2, 7, key + (7,), 0.8) * 64, dgamma0=lat((c,), 4, 15, key + (8,), 1.0) * 64,
             dbeta0=lat((c,), 4, 15, key + (9,), 1.0) * 64,
             invstd=2.0 ** torch.randint(-1, 2, (c,), generator=_seed(*key, 10)).double().numpy())
    d["gamma"] = np.where(d["gamma"] == 0, 0.25, d["gamma"])
    d["drop"] = np.array(DROP_SCALES)[torch.randint(0, 4, (N, c), generator=_seed(*key, 11)).numpy()]
    d["drop"][:2, :4] = [[2.0, 0.0, 0.5, 1.0], [0.5, 1.0, 2.0, 0.0]]
    what = f"bn {N}x{hw}x{c} act={act} res={res} drop={drop} dres={dres}"
    dr = np.repeat(d["drop"], hw, 0) if drop else 1.0
    xh = (d["x"] - d["mean"]) * d["invstd"]
    z = xh * d["gamma"] + d["beta"] + (d["res"] if res else 0.0)
    d["y"] = (z if act == ACT_NONE else np.where(z > 0, z, z * (BN_SLOPE if act == ACT_PRELU else 0.0))) * dr
    assert_fp16_exact(_t(d["y"]), what + " y")
    gg = d["dy"] * dr
    dz = gg if act == ACT_NONE else np.where(z > 0, gg, gg * (BN_SLOPE if act == ACT_PRELU else 0.0))
    d["red"] = np.concatenate([dz.sum(0), (dz * xh).sum(0)])
    _abs_sum_exact(np.abs(dz * xh).sum(0), 2.0 ** -5, what + " red")
    _abs_sum_exact(np.abs(dz).sum(0), 2.0 ** 1, what + " red")
    d["dbeta"], d["dgamma"] = d["dbeta0"] + d["red"][:c], d["dgamma0"] + d["red"][c:]
    if act == ACT_PRELU:
        d["dprelu"] = np.where(z > 0, 0.0, gg * z).sum().reshape(1)
        _abs_sum_exact(np.abs(gg * z).sum(), 2.0 ** -4, what + " dprelu")
    for k in ("red", "dbeta", "dgamma") + (("dprelu",) if act == ACT_PRELU else ()):
        assert_fp32_exact(_t(d[k]), what + " " + k)
    k1, k2 = d["red"][:c] / npix, d["red"][c:] / npix
    gi = d["gamma"] * d["invstd"]
    d["dx"] = gi * (dz - k1 - xh * k2)
    d["dx_abs"] = np.abs(gi) * (np.abs(dz) + np.abs(k1) + np.abs(xh * k2))
    d["dx_exact"] = bool((_t(d["dx"]).half().double() == _t(d["dx"])).all())
    if not d["dx_exact"]:
        assert_fp16_normal(d["dx"], BN_DX_ROUNDINGS * U * d["dx_abs"], what + " dx")
    if dres:
        d["dres"] = dz + (d["dres0"] if dres == 2 else 0.0)
        assert_fp16_exact(_t(d["dres"]), what + " dres")
    d["xh"], d["dz"] = xh, dz
    return d


def bn_dx32(d, npix):
    """the backward's dx formula evaluated operation by operation in fp32 (exact inputs: the sums in red are exact)"""
    f = np.float32
    c = d["mean"].shape[0]
    inv = f(1) / f(npix)
    k1, k2 = d["red"][:c].astype(f) * inv, d["red"][c:].astype(f) * inv
    return (d["gamma"].astype(f) * d["invstd"].astype(f)) * ((d["dz"].astype(f) - k1) - d["xh"].astype(f) * k2)


BN_MUTANTS = ["relu_one_at_zero", "drop_wrong_sample"]


def bn_mutant_applies(name, N, hw, c, act, res, drop, dres):
    return act == ACT_RELU if name == "relu_one_at_zero" else bool(drop)


def bn_mutant_red(name, N, hw, c, act, res, drop, dres):
    """red of a backward that passes the gradient at z == 0 / scales by the next sample's dropout row"""
    d = bn_case(N, hw, c, act, res, drop, dres)
    dr = np.repeat(np.roll(d["drop"], 1, 0) if name == "drop_wrong_sample" else d["drop"], hw, 0) if drop else 1.0
    z = d["xh"] * d["gamma"] + d["beta"] + (d["res"] if res else 0.0)
    gg = d["dy"] * dr
    pos = z >= 0 if name == "relu_one_at_zero" else z > 0
    dz = gg if act == ACT_NONE else np.where(pos, gg, gg * (BN_SLOPE if act == ACT_PRELU else 0.0))
    return np.concatenate([dz.sum(0), (dz * d["xh"]).sum(0)])


# (c, cstride, count, momentum)
BN_FINALIZE = [(8, 8, 4096, 0.125), (40, 48, 1024, 0.5), (5, 8, 64, 0.25)]


@functools.lru_cache(maxsize=None)
def bn_finalize_case(c, cstride, count, momentum):
    """stat = (sum, sum of squares) of ``count`` values: sums on 2^-4, so mean = sum / count is exact for a power-of-two count, and so is
    the running-mean update for a power-of-two momentum; invstd and the running variance are rounded (asked within 2 fp32 ulp)"""
    key = (c, cstride, count, int(momentum * 16), 91)
    s = lat((c,), 4, 2047, key + (1,), 1.0) * 8
    var = np.abs(lat((c,), 6, 2047, key + (2,), 1.0)) + 2.0 ** -6
    d = dict(rmean0=lat((c,), 4, 15, key + (3,), 1.0), rvar0=np.abs(lat((c,), 4, 15, key + (4,), 1.0)), eps=1e-5)
    m = s / count
    stat = np.zeros((2, cstride))
    stat[0, :c], stat[1, :c] = s, np.float32((var + m * m) * count)
    d["stat"] = stat
    v = np.maximum(stat[1, :c] / count - m * m, 0.0)
    d["mean"], d["invstd"] = m, 1.0 / np.sqrt(v + np.float64(np.float32(d["eps"])))
    d["rmean"] = (1 - momentum) * d["rmean0"] + momentum * m
    d["rvar"] = (1 - momentum) * d["rvar0"] + momentum * v * count / (count - 1)
    assert_fp32_exact(_t(d["mean"]), f"bn_finalize {c} mean")
    assert_fp32_exact(_t(d["rmean"]), f"bn_finalize {c} running mean")
    return d


def _rows_bn():
    rows = [dict(entry="csbsr_bn_apply", kernels=["bn_apply_kernel"], shape=s + cfg) for s in BN_SHAPES for cfg in BN_CONFIGS]
    bwd = ["bn_bwd_reduce_kernel", "sum_partials_kernel", "bn_bwd_apply_kernel", "bn_param_grad_kernel"]
    rows += [dict(entry="csbsr_bn_backward", kernels=bwd, shape=s + cfg)
             for s in BN_SHAPES for cfg in BN_CONFIGS]
    return rows + [dict(entry="csbsr_bn_finalize", kernels=["bn_finalize_kernel"], shape=s) for s in BN_FINALIZE]


# ------------------------------------------------------------------------------------------- channel_mean_sub

# (N, H, W, cp, step): sampled counts 64, 64 (15 -> 8 per axis: the ragged subsample), 64 at three octets, 256 at 33 octets (7 pixels per
# pass: three slices, the partial-row path), 8192 at one octet (two slices); 9 x 9 at step 1: 81 pixels, the rounded reciprocal
CMEAN = [(2, 8, 8, 8, 1), (2, 15, 15, 8, 2), (2, 16, 16, 24, 2), (2, 32, 32, 264, 2), (2, 128, 64, 8, 1), (2, 9, 9, 8, 1)]


def cmean_slices(H, W, cp, step):
    count = -(-H // step) * -(-W // step)
    P = 1 if cp // 8 >= 256 else 256 // (cp // 8)
    return count, min(max(-(-count // (P * 16)), 1), 64)


@functools.lru_cache(maxsize=None)
def cmean_case(N, H, W, cp, step):
    """x on 2^-4 {-15 .. 15}: the sum over the sampled pixels is exact, and so is the mean for a power-of-two count"""
    d = dict(x=lat((N, H, W, cp), 4, 15, (N, H, W, cp, step, 95), 0.9))
    sub = d["x"][:, ::step, ::step]
    count = sub.shape[1] * sub.shape[2]
    assert count == cmean_slices(H, W, cp, step)[0]
    assert_sum_bound(count, 15, 1, 1.0, f"channel_mean_sub {N}x{H}x{W}x{cp} step {step}")
    d["ref"] = sub.sum((1, 2)) / count
    d["exact"] = count & (count - 1) == 0
    if d["exact"]:
        assert_fp32_exact(_t(d["ref"]), f"channel_mean_sub {N}x{H}x{W}x{cp} step {step}")
    return d


def _rows_cmean():
    fold = lambda s: ["sum_partials_kernel"] if cmean_slices(*s[1:])[1] > 1 else []
    return [dict(entry="csbsr_channel_mean_sub", kernels=["channel_mean_sub_kernel"] + fold(s), shape=s)
            for s in CMEAN]


# ------------------------------------------------------------------------------------------- bilinear, ratios that round

# (N, H, W, OH, OW, align_corners, c): weights off the 1 / 16 lattice, and the one down-scale; 23 x 31 -> 50 x 70 at c = 256 takes the
# forward's column kernel
BIL_BOUNDED = [(2, H, W, OH, OW, al, 8) for H, W, OH, OW in [(5, 7, 20, 21), (23, 31, 50, 70), (6, 6, 1, 1)] for al in (0, 1)]
BIL_BOUNDED += [(2, 23, 31, 50, 70, 0, 256)]
# The kernels compute the source position in fp32: in / out, its product with o + .5, the - .5 (align_corners: one division): at most three
# roundings of a number below ``in``, so the position is off by at most 3 x 2^-24 x in per axis.  The interpolant is piecewise linear in
# the position with slope |x_a - x_b| of neighbouring pixels, and a position that close to an integer may pick the neighbouring pair: the
# result moves by at most 3 (H + W) 2^-24 T, T = the sum of |x| over the 4 x 4 pixels round the source position (rows / columns
# i0 - 1 .. i0 + 2, clipped).  The arithmetic: 1 - wx, 1 - wy, four products and an addition per row pair, two products and the last
# addition, the dropout scale: 12 roundings, each of at most T.  Backward: the same position error moves every weight of the K outputs
# within two pixels of the input pixel (T = the sum of |dy| over them (+ |dx0|)); per term 1 - w twice, cy cx, its product with g, and
# at most K additions, the dropout scale, the add onto dx0.
BIL_FWD_ROUNDINGS = 12


def bil_roundings(direction, H, W, K=0):
    return (BIL_FWD_ROUNDINGS if direction == "fwd" else K + 8) + 3 * (H + W)


def bil_src(o, n_in, n_out, align, f=np.float64):
    """(i0, i1, w1) of output o, every operation in the float type ``f`` (np.float32: bil_src of the kernels, operation by operation)"""
    if align:
        src = f(o) * f(n_in - 1) / f(n_out - 1) if n_out > 1 else f(0)
    else:
        src = max((f(o) + f(0.5)) * (f(n_in) / f(n_out)) - f(0.5), f(0))
    i0 = min(int(src), n_in - 1)
    return i0, min(i0 + 1, n_in - 1), src - f(i0)


def bil_matrix32(n_in, n_out, align):
    """the two-tap matrix with the kernels' fp32 source positions and the fp32 value of 1 - w"""
    M = np.zeros((n_out, n_in), np.float32)
    for o in range(n_out):
        i0, i1, w1 = bil_src(o, n_in, n_out, align, np.float32)
        M[o, i0] += np.float32(1) - w1
        M[o, i1] += w1
    return M


def bil_near(n_in, n_out, align):
    """0 / 1 [n_out, n_in]: the pixels i0 - 1 .. i0 + 2 (clipped) round output o's source position"""
    E = np.zeros((n_out, n_in))
    for o in range(n_out):
        i0 = bil_src(o, n_in, n_out, align)[0]
        E[o, max(i0 - 1, 0):min(i0 + 3, n_in)] = 1.0
    return E


@functools.lru_cache(maxsize=4)
def bilinear_bounded_case(N, H, W, OH, OW, align, c):
    """x, dy, dx0 on 2^-4 {-15 .. 15} (fp16 values; nothing here is exact), the dropout rows of bilinear_case"""
    key = (N, H, W, OH, OW, align, c, 53)
    My, Mx, Ey, Ex = bil_matrix(H, OH, align), bil_matrix(W, OW, align), bil_near(H, OH, align), bil_near(W, OW, align)
    d = dict(x=lat((N, H, W, c), 4, 15, key + (1,), 0.9), dy=lat((N, OH, OW, c), 4, 15, key + (2,), 0.9), dx0=lat((N, H, W, c), 4, 15, key + (3,), 0.9))
    d["drop"] = np.array(DROP_SCALES)[torch.randint(0, 4, (N, c), generator=_seed(*key, 4)).numpy()]
    d["drop"][:2, :4] = [[2.0, 0.0, 0.5, 1.0], [0.5, 1.0, 2.0, 0.0]]
    d["y"], d["dx"] = bil_apply(My, d["x"], Mx), bil_apply(My.T, d["dy"], Mx.T)
    d["y_T"], d["dx_T"] = bil_apply(Ey, np.abs(d["x"]), Ex), bil_apply(Ey.T, np.abs(d["dy"]), Ex.T)
    d["K"] = int(Ey.sum(0).max() * Ex.sum(0).max())
    My32, Mx32 = bil_matrix32(H, OH, align), bil_matrix32(W, OW, align)
    f = np.float32
    d["y32"] = np.einsum("pw,nowc->nopc", Mx32, np.einsum("oh,nhwc->nowc", My32, d["x"].astype(f)))
    d["dx32"] = np.einsum("wp,nopc->nowc", Mx32.T, np.einsum("ho,nopc->nhpc", My32.T, d["dy"].astype(f)))
    assert d["y32"].dtype == f and d["dx32"].dtype == f
    return d


def bilinear_bounds(d, direction, drop, accumulate, H, W):
    """(fp64 reference, the fp32 part of the bound) of one bounded bilinear row"""
    dr = d["drop"][:, None, None, :] if drop else 1.0
    if direction == "fwd":
        return d["y"] * dr, bil_roundings("fwd", H, W) * U * d["y_T"] * np.abs(dr)
    ref = d["dx"] * dr + (d["dx0"] if accumulate else 0.0)
    return ref, bil_roundings("bwd", H, W, d["K"]) * U * (d["dx_T"] * np.abs(dr) + (np.abs(d["dx0"]) if accumulate else 0.0))


def bilinear_bounded_mutant(name, direction, N, H, W, OH, OW, align, c):
    """no_half_pixel / bwd_misses_last of bilinear_mutant on the bounded rows' inputs (no dropout row)"""
    d = bilinear_bounded_case(N, H, W, OH, OW, align, c)
    My, Mx = bil_matrix(H, OH, align), bil_matrix(W, OW, align)
    if name == "no_half_pixel":
        My, Mx = bil_matrix(H, OH, 0, half_pixel=False), bil_matrix(W, OW, 0, half_pixel=False)
    else:
        Mx = bil_matrix(W, OW, align, drop_last=True)
    return bil_apply(My, d["x"], Mx) if direction == "fwd" else bil_apply(My.T, d["dy"], Mx.T)


# (planes, H, W, OH, OW, align_corners) of csbsr_bilinear32_fwd / _bwd (csrc/image_ops.hip: fp32 planes, one kernel each way)
BIL32_EXACT = [(3, 5, 7, 10, 14, 0), (3, 5, 9, 9, 33, 1), (2, 1, 1, 8, 8, 0), (2, 4, 4, 32, 32, 0)]
BIL32_BOUNDED = [(3, H, W, OH, OW, al) for H, W, OH, OW in [(5, 7, 20, 21), (23, 31, 50, 70), (6, 6, 1, 1)] for al in (0, 1)]


@functools.lru_cache(maxsize=None)
def bilinear32_case(planes, H, W, OH, OW, align):
    """the fp16 rows' construction on fp32 planes [planes, H, W]: integers in {-7 .. 7} on the exact rows (every sum on 2^-8, proved
    fp32-exact), 2^-4 {-15 .. 15} on the bounded ones (the same bounds without the dropout scale, the accumulation and the fp16 store)"""
    key = (planes, H, W, OH, OW, align, 57)
    exact = (planes, H, W, OH, OW, align) in BIL32_EXACT
    My, Mx = bil_matrix(H, OH, align), bil_matrix(W, OW, align)
    q, amp = (0, 7) if exact else (4, 15)
    d = dict(x=lat((planes, H, W), q, amp, key + (1,), 0.9), dy=lat((planes, OH, OW), q, amp, key + (2,), 0.9), exact=exact)
    ap = lambda A, v, B: np.einsum("pw,now->nop", B, np.einsum("oh,nhw->now", A, v))
    d["y"], d["dx"] = ap(My, d["x"], Mx), ap(My.T, d["dy"], Mx.T)
    if exact:
        for M in (My, Mx):
            assert_on_lattice(_t(M), 2.0 ** -4, f"bilinear32 {key} weights")
        assert_sum_bound(int((My != 0).sum(0).max() * (Mx != 0).sum(0).max()) + 1, 7, 2.0 ** 8, 1.0, f"bilinear32 {key}")
        assert_fp32_exact(_t(d["y"]), f"bilinear32 {key} y")
        assert_fp32_exact(_t(d["dx"]), f"bilinear32 {key} dx")
        return d
    Ey, Ex = bil_near(H, OH, align), bil_near(W, OW, align)
    K = int(Ey.sum(0).max() * Ex.sum(0).max())
    d["y_bound"] = bil_roundings("fwd", H, W) * U * ap(Ey, np.abs(d["x"]), Ex)
    d["dx_bound"] = bil_roundings("bwd", H, W, K) * U * ap(Ey.T, np.abs(d["dy"]), Ex.T)
    My32, Mx32 = bil_matrix32(H, OH, align), bil_matrix32(W, OW, align)
    d["y32"], d["dx32"] = ap(My32, d["x"].astype(np.float32), Mx32), ap(My32.T, d["dy"].astype(np.float32), Mx32.T)
    return d


def _rows_bilinear32():
    """(these two live in csrc/image_ops.hip, outside the source the coverage check parses; listed so that the tables name them)"""
    return [dict(entry=f"csbsr_bilinear32_{d}", kernels=[f"bilinear32_{d}_kernel"], shape=s) for s in BIL32_EXACT + BIL32_BOUNDED for d in ("fwd", "bwd")]


def _rows_bilinear_bounded():
    rows = []
    for s in BIL_BOUNDED:
        N, H, W, OH, OW, al, c = s
        rows.append(dict(entry="csbsr_bilinear_fwd", kernels=bilinear_kernel_for("fwd", N, H, W, OH, OW, c), shape=s))
        rows.append(dict(entry="csbsr_bilinear_bwd", kernels=bilinear_kernel_for("bwd", N, H, W, OH, OW, c), shape=s))
    return rows


# ------------------------------------------------------------------------------------------- max pool 3x3 s2 p1, plain entry points

# (N, H, W, c): one pixel; H = 1 and W = 1 (every window cut to one row / column); odd and even sizes; three octets
MAXPOOL = [(2, 1, 1, 8), (2, 1, 7, 8), (2, 6, 1, 8), (2, 5, 6, 24), (2, 8, 9, 8)]


def maxpool_ref(x, dy=None, last=False):
    """y [N, OH, OW, c] and, with dy, dx: each window's gradient goes to its FIRST maximum in scan order (torch's rule; ``last``: the
    mutant that takes the last one)"""
    N, H, W, c = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y, dx = np.zeros((N, OH, OW, c)), np.zeros((N, H, W, c))
    n_i, c_i = np.meshgrid(np.arange(N), np.arange(c), indexing="ij")
    for oy in range(OH):
        for ox in range(OW):
            pos = [(iy, ix) for iy in range(2 * oy - 1, 2 * oy + 2) for ix in range(2 * ox - 1, 2 * ox + 2) if 0 <= iy < H and 0 <= ix < W]
            win = np.stack([x[:, iy, ix] for iy, ix in pos])          # [taps, N, c]
            y[:, oy, ox] = win.max(0)
            if dy is not None:
                arg = (len(pos) - 1 - win[::-1].argmax(0)) if last else win.argmax(0)
                iy, ix = np.array(pos)[arg].transpose(2, 0, 1)
                np.add.at(dx, (n_i, iy, ix, c_i), dy[:, oy, ox])
    return y, dx


@functools.lru_cache(maxsize=None)
def maxpool_case(N, H, W, c):
    """x integers in {-2 .. 2}: nearly every window holds ties; dy on 2^-4 {-15 .. 15}: a pixel collects at most four windows"""
    key = (N, H, W, c, 59)
    d = dict(x=lat((N, H, W, c), 0, 2, key + (1,), 0.8), dy=lat((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, c), 4, 15, key + (2,), 1.0))
    d["y"], d["dx"] = maxpool_ref(d["x"], d["dy"])
    assert_fp16_exact(_t(d["dx"]), f"maxpool {key} dx")
    return d


def _rows_maxpool():
    return ([dict(entry="csbsr_maxpool3x3s2_fwd", kernels=["maxpool_fwd_kernel"], shape=s) for s in MAXPOOL]
            + [dict(entry="csbsr_maxpool3x3s2_bwd", kernels=["maxpool_bwd_kernel"], shape=s) for s in MAXPOOL])


# ------------------------------------------------------------------------------------------- instance-norm backward

INSTNORM_CHUNK = 65536
# (N, C, hw): hw on both sides of the 65536-pixel chunk rule (one partial row per plane, and two)
INSTNORM = [(2, C, hw) for C in (1, 3) for hw in (100, INSTNORM_CHUNK, INSTNORM_CHUNK + 1)]
# every rounding of the apply kernel's sequence for one element: x - mean and its product with invstd (xh), red0 / hw, xh red1 and its
# division by hw, the two subtractions, the product with invstd -- eight, and the add onto dx0; each at most 2^-24 of
# invstd (|g| + |red0 / hw| + |xh red1 / hw|) (+ |dx0|)
INSTNORM_ROUNDINGS = 8


@functools.lru_cache(maxsize=None)
def instnorm_case(N, C, hw):
    """x, mean on 2^-4 {-7 .. 7}, invstd in {1/2, 1, 2}, g on 2^-2 {-1, 0, 1} in the first C lanes of an 8-lane pixel (the other lanes
    hold values that must not reach a sum): red is exact; dx rounds (hw need not be a power of two)"""
    key = (N, C, hw, 97)
    d = dict(x=lat((N, C, hw), 4, 7, key + (1,), 0.9), mean=lat((N, C), 4, 7, key + (2,), 1.0), dy8=lat((N, hw, 8), 2, 1, key + (3,), 0.8),
             dx0=lat((N, C, hw), 4, 15, key + (4,), 0.9), invstd=2.0 ** torch.randint(-1, 2, (N, C), generator=_seed(*key, 5)).double().numpy())
    g = d["dy8"][..., :C].transpose(0, 2, 1)
    xh = (d["x"] - d["mean"][..., None]) * d["invstd"][..., None]
    what = f"instnorm_bwd {N}x{C}x{hw}"
    d["red"] = np.stack([g.sum(2), (g * xh).sum(2)], -1)
    _abs_sum_exact(np.abs(g * xh).sum(2), 2.0 ** -7, what + " red")
    assert_fp32_exact(_t(d["red"]), what + " red")
    k1, k2 = d["red"][..., 0:1] / hw, xh * d["red"][..., 1:2] / hw
    d["dx"] = d["invstd"][..., None] * (g - k1 - k2)
    d["dx_abs"] = d["invstd"][..., None] * (np.abs(g) + np.abs(k1) + np.abs(k2))
    d["g"], d["xh"] = g, xh
    return d


def instnorm_bound(d, accumulate):
    return (INSTNORM_ROUNDINGS + (1 if accumulate else 0)) * U * (d["dx_abs"] + (np.abs(d["dx0"]) if accumulate else 0.0))


def instnorm_dx32(d, hw, accumulate):
    """the apply kernel's formula operation by operation in fp32"""
    f = np.float32
    g, xh, red, is_ = d["g"].astype(f), d["xh"].astype(f), d["red"].astype(f), d["invstd"].astype(f)[..., None]
    v = is_ * ((g - red[..., 0:1] / f(hw)) - (xh * red[..., 1:2]) / f(hw))
    return d["dx0"].astype(f) + v if accumulate else v


def _rows_instnorm():
    kernels = ["instnorm_bwd_reduce_kernel", "sum_partials_kernel", "instnorm_bwd_apply_kernel"]
    return [dict(entry="csbsr_instnorm_bwd", kernels=kernels, shape=s) for s in INSTNORM]


# ------------------------------------------------------------------------------------------- coverage

@functools.lru_cache(maxsize=None)
def rows():
    return (_rows_border() + _rows_wpool() + _rows_aap() + _rows_bilinear() + _rows_epilogue() + _rows_small() + _rows_bn() + _rows_cmean()
            + _rows_bilinear_bounded() + _rows_bilinear32() + _rows_maxpool() + _rows_instnorm())


# names asserted by another exact suite (the file that asserts them bit for bit or against a counted bound)
COVERED_ELSEWHERE = {
    "csbsr_set_reduction_scratch": "test_image_exact_gpu.py",          # test_aa_down_bwd_without_scratch unregisters and re-registers it
    "csbsr_plane_reduce": "test_metrics_exact_gpu.py",
    "plane_reduce_kernel": "test_metrics_exact_gpu.py",
    "csbsr_axpby_split": "test_split_planes_gpu.py",
    "csbsr_sum_act_split": "test_split_planes_gpu.py",
    "csbsr_weighted_pool_fwd_split": "test_split_planes_gpu.py",
    "csbsr_nchw32_to_nhwc16_split": "test_split_planes_gpu.py",
    "csbsr_maxpool3x3s2_fwd_split": "test_split_planes_gpu.py",
    "csbsr_maxpool3x3s2_bwd_split": "test_split_planes_gpu.py",
    "csbsr_adaptive_avgpool_fwd_split": "test_split_planes_gpu.py",
    "csbsr_bilinear_fwd_split": "test_split_planes_gpu.py",
}
_RELMAX = "no exact row yet: still held only to the relmax tolerance of test_elementwise_gpu.py"
# name -> the written reason why it has no row here
NOT_COVERED = {
    "csbsr_round_weights": "keeps its property test (test_elementwise_gpu.py): the result is a choice among fp16 neighbours, not a sum",
    "round_weights_kernel": "keeps its property test (test_elementwise_gpu.py), as csbsr_round_weights",
    "round_weights_reg_kernel": "keeps its property test (test_elementwise_gpu.py), as csbsr_round_weights",
    "round_weights_lanes_kernel": "keeps its property test (test_elementwise_gpu.py), as csbsr_round_weights",
}


def source_names(text=None):
    """every extern "C" entry point and every __global__ kernel name of csrc/elementwise.hip"""
    text = source() if text is None else text
    entries = re.findall(r'extern "C" int (csbsr_\w+)\(', text)
    kernels = re.findall(r"__global__(?: __launch_bounds__\(\d+\))? void (\w+)\(", text)
    assert len(kernels) == len(re.findall(r"__global__", text)), "a __global__ line the pattern does not parse"
    assert len(entries) == len(re.findall(r'extern "C"', text)), 'an extern "C" line the pattern does not parse'
    return entries, kernels


def missing_names(table=None, elsewhere=None, not_covered=None, text=None):
    """the names of the source that no row, no other suite and no written reason accounts for"""
    table = rows() if table is None else table
    elsewhere = COVERED_ELSEWHERE if elsewhere is None else elsewhere
    not_covered = NOT_COVERED if not_covered is None else not_covered
    named = {r["entry"] for r in table} | {k for r in table for k in r["kernels"]}
    entries, kernels = source_names(text)
    return [n for n in entries + kernels if n not in named and n not in elsewhere and n not in not_covered]
