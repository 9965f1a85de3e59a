"""Shared by tests/test_edt_cases_cpu.py and tests/test_edt_exact_gpu.py: references, a numpy model of the block-bounded row search and
the geometry table for the exact Euclidean distance transform of csrc/image_ops.hip -- edt_cols_kernel, edt_rows_kernel and
sdf_combine_kernel behind csbsr_sdf, crack_cols_kernel and crack_rows_weight_kernel behind csbsr_crack_weight.  No GPU.

References
  d2_exact(fg)          integer squared distance of every pixel to the nearest False pixel (int64; NONE where the image has no False
                        pixel): scipy.ndimage.distance_transform_edt squared and rounded, cross-checked on the small rows against
                        d2_brute, an O(n^2) enumeration in integers.
  sdf_restated32(mask)  the kernel as written, in float32: foreground = the value truncated to uint8 is non-zero; pos = sqrt(float32(d2))
                        to the nearest background pixel, neg to the nearest foreground pixel; the maxima pmax, nmax per sample;
                        neg / nmax - pos / pmax; the inner boundary (foreground pixels with a background pixel among their four
                        neighbours, borders clamped) set to 0.  A sample without foreground is 0 (pmax = 0).  A sample of NOTHING BUT
                        foreground is -1 everywhere: no pixel has a background pixel to measure to, every pos is the row pass's "none"
                        (sqrt(1e18f)) and so is pmax, pos / pmax = 1; nmax = 0 and the kernel puts 0 for the outside term where the
                        reference divides 0 / 0 and returns NaN.
  sdf_ref64(mask)       oracle.csbsr_oracle.compute_sdf (float64, scipy).
  the weight            crack_weight_cases.distance (float64) and, for the mutants, weight_from_d2.

The counted bound (sdf_bound)
  At every pixel one of the two terms of neg / nmax - pos / pmax is zero (pos = 0 on background, neg = 0 on foreground), so the
  subtraction is exact and |sdf| = q = d / m with m the sample's maximum of that distance, q <= 1.  In float32, on a row with
  H^2 + W^2 < 2^24 (exact = True): d2 is an integer below 2^24, held exactly; d = sqrt(d2) rounds once (correctly: v_sqrt_f32 with its
  fix-up); m is the maximum of such roots, one rounding of its own; the division rounds once (correctly).  Three relative errors of
  u = 2^-24 each on a value of at most 1:  |sdf32 - sdf| <= 3 u + O(u^2), counted as 3 * 2^-24 + 2^-44 (the second-order terms 3 u^2 and
  the float64 reference's own 3 * 2^-53).  On the other rows (W > 4095) the squares (x - x')^2 and the sums g^2 + (x - x')^2 round too: the
  kernel finds the minimum of sums that are each within (1 + u)^2 of the exact one, so d2 carries 2 u, its root one more u on d -- and the
  same on m: 5 * 2^-24 + 2^-44.  The inner boundary and the all-background sample are exact zeros.

The model (model_d2) restates the device code in int64: the two column scans, the squares of a row, the minima of its 32-column blocks,
the scan of the own block, then blocks bx - d / bx + d with the gaps x - (32 bl + 31) / 32 br - x, the strict < tests and the break
when neither side is in range and in reach.  Its ``defect`` switches produce the mutants of MUTANTS; the CPU tests prove through the
comparison functions below (the ones the GPU test uses) that each is caught by the row named for it.
"""
import functools

import numpy as np

import crack_weight_cases as CW

f32 = np.float32
U = 2.0 ** -24
NONE = 10 ** 18                          # squared distance where there is no pixel to measure to (the device's 1e18f)
FP32_EXACT = 1 << 24
LAMBDA = CW.LAMBDA
WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 513, 1000)
HEIGHTS = (1, 2, 3, 40)
MAX_W = 8192                             # the widest row the two entry points accept
SOFT_VALUES = (0.5, 0.99, 1.0, 1.5, 254.9, 1e-40, -0.0)
D2_RESOLVED = 1 << 21                    # an error of 1 in d2 shows in the weight check wherever d2 <= this (see weight_amp)


# ------------------------------------------------------------------------------------------- references

def foreground(mask):
    """the reference's rule: the value truncated to uint8 is non-zero"""
    return CW.foreground(np.asarray(mask, f32))


def d2_exact(fg):
    """[H, W] bool -> int64 squared distance to the nearest False pixel, NONE everywhere if there is none"""
    from scipy.ndimage import distance_transform_edt
    fg = np.asarray(fg, bool)
    if fg.all():
        return np.full(fg.shape, NONE, np.int64)
    d = distance_transform_edt(fg)
    return np.rint(d * d).astype(np.int64)


def d2_brute(fg):
    """the same by enumeration in integers"""
    fg = np.asarray(fg, bool)
    H, W = fg.shape
    zy, zx = np.nonzero(~fg)
    if zy.size == 0:
        return np.full(fg.shape, NONE, np.int64)
    out = np.empty(H * W, np.int64)
    yy, xx = np.divmod(np.arange(H * W), W)
    for i in range(0, H * W, 2048):
        dy = yy[i:i + 2048, None] - zy[None, :]
        dx = xx[i:i + 2048, None] - zx[None, :]
        out[i:i + 2048] = (dy * dy + dx * dx).min(1)
    return out.reshape(H, W)


def _root32(d2):
    return np.sqrt(np.where(d2 >= NONE // 10, f32(1e18), d2.astype(f32)).astype(f32))


def sdf_from_d2(fg, pos2, neg2, batch_max=False, eight=False):
    """the combine pass in float32: fg [N, H, W] bool, pos2 / neg2 [N, H, W] int64 -> [N, 1, H, W] float32"""
    pos, neg = _root32(pos2), _root32(neg2)
    N = fg.shape[0]
    pmax, nmax = pos.reshape(N, -1).max(1), neg.reshape(N, -1).max(1)
    if batch_max:
        pmax, nmax = np.full(N, pmax.max(), f32), np.full(N, nmax.max(), f32)
    out = np.zeros(fg.shape, f32)
    for n in range(N):
        if not pmax[n] > 0:
            continue
        nterm = neg[n] / nmax[n] if nmax[n] > 0 else np.zeros_like(neg[n])
        v = (nterm - pos[n] / pmax[n]).astype(f32)
        p = np.pad(fg[n], 1, mode="edge")
        inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
        if eight:
            inner = inner & p[:-2, :-2] & p[:-2, 2:] & p[2:, :-2] & p[2:, 2:]
        v[fg[n] & ~inner] = 0
        out[n] = v
    return out[:, None]


def sdf_restated32(mask):
    fg = foreground(mask)[:, 0]
    pos2 = np.stack([d2_exact(f) for f in fg])
    neg2 = np.stack([d2_exact(~f) for f in fg])
    return sdf_from_d2(fg, pos2, neg2)


def sdf_ref64(mask):
    from oracle import csbsr_oracle as O
    with np.errstate(invalid="ignore", divide="ignore"):
        return O.compute_sdf(np.asarray(mask, f32))


def all_foreground(mask):
    """[N] bool: the samples of nothing but foreground (the reference is NaN there)"""
    fg = foreground(mask)
    return fg.reshape(fg.shape[0], -1).all(1)


def is_exact(H, W):
    return H * H + W * W < FP32_EXACT


def sdf_bound(exact):
    return (3 if exact else 5) * U + 2.0 ** -44


def weight_from_d2(fg, d2, amp, lam=LAMBDA):
    """lambda exp(-amp sqrt(d2)) in float64 from squared distances to the nearest foreground pixel [N, H, W]; lambda for a sample
    without foreground"""
    d = np.sqrt(np.where(d2 >= NONE // 10, 0, d2).astype(np.float64))
    return (lam * np.exp(-float(f32(amp)) * d))[:, None]


# ------------------------------------------------------------------------------------------- the model of the device search

DEFECTS = ("far_edge", "break_either", "ragged32", "no_own", "cols_one_way")
_BIG = 10 ** 9


def model_cols(fg, one_way=False):
    """[N, H, W] bool -> int64 vertical distance to the nearest False pixel of the column (>= 10^9 where it has none): the two scans"""
    N, H, W = fg.shape
    g = np.empty((N, H, W), np.int64)
    d = np.full((N, W), _BIG, np.int64)
    for y in range(H):
        d = np.where(fg[:, y], d + 1, 0)
        g[:, y] = d
    if not one_way:
        d = np.full((N, W), _BIG, np.int64)
        for y in range(H - 1, -1, -1):
            d = np.where(fg[:, y], d + 1, 0)
            g[:, y] = np.minimum(g[:, y], d)
    return g


def model_rows(g, defect=None):
    """[R, W] int64 column distances -> int64 min over x' of g(x')^2 + (x - x')^2 by the device's search order"""
    R, W = g.shape
    nb = (W + 31) >> 5
    sq = np.where(g >= 10 ** 8, NONE, g * g)
    ext = np.full((R, 32 * nb), NONE, np.int64)          # the row as the scans see it: nothing beyond column W - 1 ...
    ext[:, :W] = sq
    bmin = ext.reshape(R, nb, 32).min(2)
    if defect == "ragged32":                             # ... or, with the ragged block scanned over 32 columns, what lies behind the
        k = 32 * nb - W                                  # row in LDS: the block minima
        ext[:, W:] = bmin[:, :k] if k <= nb else np.concatenate([bmin, np.full((R, k - nb), NONE, np.int64)], 1)
        bmin = ext.reshape(R, nb, 32).min(2)
    best = sq.copy()
    lane = np.arange(32)

    def scan(r, x, b):
        cols = 32 * b[:, None] + lane[None, :]
        dd = x[:, None] - cols
        cand = (ext[r[:, None], cols] + dd * dd).min(1)
        best[r, x] = np.minimum(best[r, x], cand)

    r, x = (a.reshape(-1) for a in np.meshgrid(np.arange(R), np.arange(W), indexing="ij"))
    bx = x >> 5
    if defect != "no_own":
        own = bmin[r, bx] < best[r, x]
        scan(r[own], x[own], bx[own])
    for d in range(1, nb):
        if r.size == 0:
            break
        bl, br = bx - d, bx + d
        if defect == "far_edge":
            gl, gr = x - 32 * bl, 32 * br + 31 - x
        else:
            gl, gr = x - (32 * bl + 31), 32 * br - x
        cur = best[r, x]
        lin = (bl >= 0) & (gl * gl < cur)
        rin = (br < nb) & (gr * gr < cur)
        alive = (lin & rin) if defect == "break_either" else (lin | rin)
        r, x, bx, bl, br, gl, gr, lin, rin = (a[alive] for a in (r, x, bx, bl, br, gl, gr, lin, rin))
        go = lin.copy()
        go[lin] = bmin[r[lin], bl[lin]] + gl[lin] ** 2 < best[r[lin], x[lin]]
        scan(r[go], x[go], bl[go])
        go = rin.copy()
        go[rin] = bmin[r[rin], br[rin]] + gr[rin] ** 2 < best[r[rin], x[rin]]
        scan(r[go], x[go], br[go])
    return np.where(best >= NONE // 10, NONE, best)


def model_d2(fg, defect=None):
    """[N, H, W] bool -> int64 squared distance to the nearest False pixel as the device computes it (NONE: no such pixel)"""
    fg = np.asarray(fg, bool)
    N, H, W = fg.shape
    g = model_cols(fg, one_way=defect == "cols_one_way")
    return model_rows(g.reshape(N * H, W), defect).reshape(N, H, W)


MUTANTS = {          # name -> (what is wrong, the rows that must catch it)
    "far_edge": ("the gap is measured to the far edge of the block", ("equal_reach", "near_tradeoff")),
    "break_either": ("the search stops when either side fails", ("break_left", "break_right")),
    "ragged32": ("the ragged last block is scanned over 32 columns", ("lone_feature",)),
    "no_own": ("the own block is not scanned", ("w33_h3", "near_tradeoff")),
    "cols_one_way": ("the column pass runs in one direction only", ("near_tradeoff", "w32_h40")),
    "batch_max": ("the maximum is taken over the batch", ("n3_extents",)),
    "eight": ("the inner boundary looks at eight neighbours", ("n3_extents", "seeded_sparse")),
    "ne0": ("foreground is ``!= 0`` (the kernel before the truncation rule)", ("soft_values", "soft_halo", "seeded_sparse")),
}
WEIGHT_MUTANTS = ("far_edge", "break_either", "ragged32", "no_own", "cols_one_way", "ne0")


def mutant_sdf(mask, name):
    """csbsr_sdf with the defect ``name`` -> [N, 1, H, W] float32"""
    mask = np.asarray(mask, f32)
    fg = (mask != 0)[:, 0] if name == "ne0" else foreground(mask)[:, 0]
    defect = name if name in DEFECTS else None
    return sdf_from_d2(fg, model_d2(fg, defect), model_d2(~fg, defect), batch_max=name == "batch_max", eight=name == "eight")


def mutant_weight(mask, name, amp):
    """csbsr_crack_weight with the defect ``name`` -> [N, 1, H, W] float32"""
    mask = np.asarray(mask, f32)
    fg = (mask != 0)[:, 0] if name == "ne0" else foreground(mask)[:, 0]
    return weight_from_d2(fg, model_d2(~fg, name if name in DEFECTS else None), amp).astype(f32)


# ------------------------------------------------------------------------------------------- the geometry table

def _fix_extremes(m):
    """no sample of nothing but foreground; a sample of nothing but background only where the image has a single pixel"""
    for s in m[:, 0]:
        if s.all():
            s[0, 0] = 0
        if not s.any() and s.size > 1:
            s[-1, -1] = 1
    return m


def _width_mask(H, W):
    """two samples: a sparse one (a few features, most columns without any) and a dense one (a few holes)"""
    rng = np.random.default_rng(1000 * H + W)
    m = np.zeros((2, 1, H, W), f32)
    m[0, 0] = rng.random((H, W)) < min(0.5, 2.0 / W)
    m[1, 0] = rng.random((H, W)) < 0.85
    return _fix_extremes(m)


def _lone_feature():
    W = 1000
    cols = (0, 31, 32, 63, W - 1, 994)          # 994: the only feature sits in the ragged last block (992 .. 999)
    m = np.zeros((len(cols), 1, 2, W), f32)
    for n, c in enumerate(cols):
        m[n, 0, n % 2, c] = 1
    return m


def _equal_reach():
    m = np.zeros((2, 1, 1, 1000), f32)
    m[0, 0, 0, [400, 600]] = 1                  # x = 500 (block 15): blocks 12 and 18, 100 columns either way
    m[1, 0, 0, [95, 96, 417]] = 1               # x = 256: 160 and 161 columns; the left one wins by a column
    return m


def _near_tradeoff():
    k, W, c = 33, 257, 100
    m = np.zeros((3, 1, k + 1, W), f32)
    for n, off in enumerate((k - 1, k, k + 1)):
        m[n, 0, k, c] = 1                       # from (0, c): k rows down ...
        m[n, 0, 0, c + off] = 1                 # ... against g = 0, k - 1 / k / k + 1 columns away (gap^2 == best at k)
    return m


def _empty_cols():
    m = np.zeros((1, 1, 4, 513), f32)
    rng = np.random.default_rng(7)
    m[0, 0, :, :20] = rng.random((4, 20)) < 0.3
    m[0, 0, 2, 330:340] = 1                     # blocks 1 .. 9 and 11 .. 16 have no feature at all
    m[0, 0, 0, 3] = 1
    return m


def _break(left):
    W = 1000
    m = np.zeros((1, 1, 1, W), f32)
    m[0, 0, 0, W - 3 if left else 2] = 1
    return m


def _complement():
    m = np.zeros((2, 1, 7, 70), f32)
    m[0] = 1
    m[0, 0, 3, 40] = 0
    m[1, 0, 5, 66] = 1
    return m


def _n3_extents():
    m = np.zeros((3, 1, 5, 300), f32)
    m[0, 0, 4, 299] = 1
    m[1, 0] = np.random.default_rng(11).random((5, 300)) < 0.6
    m[1, 0, 1:4, 100:140] = 1                   # a block with an interior: its inner boundary has diagonal-only neighbours at the corners
    m[1, 0, 2, 120] = 0
    return m


def _all_foreground():
    m = np.ones((2, 1, 5, 40), f32)
    m[1, 0, 2, 7:30] = 0
    return m


def _soft_values():
    """sample 0: a {0, 1} crack and every soft value on its own, away from it; sample 1: soft values only, all below 1 (no foreground
    for the reference, nothing but foreground for ``!= 0``); sample 2: every value of the domain's ends"""
    m = np.zeros((3, 1, 6, 40), f32)
    m[0, 0, 2:4, 5:12] = 1
    for i, v in enumerate(SOFT_VALUES):
        m[0, 0, 1 + (i % 2) * 3, 15 + 3 * i] = v
    m[1, 0] = np.where(np.random.default_rng(3).random((6, 40)) < 0.5, f32(0.5), f32(0.99))
    m[1, 0, 0, :3] = (f32(1e-40), f32(-0.0), f32(0.999999))
    m[2, 0] = np.random.default_rng(4).random((6, 40)).astype(f32) * f32(1.2)          # about one in six is >= 1
    m[2, 0, 5, :4] = (f32(255.99), f32(254.9), f32(1.0), f32(0.0))
    return m


def _soft_halo():
    m = np.zeros((1, 1, 9, 65), f32)
    m[0, 0, 3:6, 10:50] = 1
    halo = np.zeros((9, 65), bool)
    halo[2:7, 9:51] = True
    m[0, 0][halo & (m[0, 0] == 0)] = 0.5
    return m


def _seeded_sparse():
    import torch
    import torch.nn.functional as F
    from csbsr_amd.data.synthetic import crack_masks
    m = crack_masks(2, 96, 200, torch.Generator().manual_seed(3))
    ys, xs = np.nonzero(m[1, 0].numpy())          # a window round the crack, 4 pixels of margin, stretched to the full size
    win = m[1:2, :, max(0, ys.min() - 4):ys.max() + 5, max(0, xs.min() - 4):xs.max() + 5]
    soft = F.interpolate(win, size=(96, 200), mode="bilinear", align_corners=False)
    return torch.cat([m[:1], soft]).numpy().astype(f32)


def _big_5():
    """tests/test_elementwise_gpu.py's wide sparse batch, its all-foreground sample replaced by a full one with a single hole"""
    H, W = 96, 1000
    m = np.zeros((5, 1, H, W), f32)
    m[0, 0, 40:43, 700:960] = 1
    m[0, 0, 5:90, 17] = 1
    m[1, 0, H - 1, W - 1] = 1
    m[2, 0, 10:12, :] = 1
    m[4] = 1
    m[4, 0, 50, 333] = 0
    return m


def _blobs(H, W, n, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((1, 1, H, W), f32)
    for _ in range(n):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        m[0, 0, y:y + int(rng.integers(1, 6)), x:x + int(rng.integers(1, 30))] = 1
    return m


def _full_sparse():
    """bench-like: three thin cracks of about 80 pixels in a 64 x 1792 image, about 0.4 % foreground"""
    H, W = 64, 1792
    rng = np.random.default_rng(17)
    m = np.zeros((1, 1, H, W), f32)
    for x0 in (150, 900, 1500):
        y = float(rng.integers(10, H - 10))
        for t in range(80):
            y = min(max(y + float(rng.normal(0, 0.6)), 0), H - 2)
            m[0, 0, int(y):int(y) + 2, x0 + t] = 1
    return m


def _wide(H, W, cols):
    m = np.zeros((1, 1, H, W), f32)
    for i, c in enumerate(cols):
        m[0, 0, i % H, c] = 1
    return m


def _table():
    rows = []

    def add(name, cls, build, why):
        m = build()
        N, _, H, W = m.shape
        rows.append(dict(name=name, cls=cls, N=N, H=H, W=W, build=build, why=why, exact=is_exact(H, W)))

    for W in WIDTHS:
        for H in HEIGHTS:
            add(f"w{W}_h{H}", "width", functools.partial(_width_mask, H, W),
                f"width {W} (blocks of 32, the 256-lane stride) at height {H}: a sparse and a dense random sample")
    add("big_5x96x1000", "largest", _big_5, "wide sparse batch: a band, a column, a corner pixel, a full-width stripe, an empty sample, one hole")
    add("big_1x200x1000", "largest", functools.partial(_blobs, 200, 1000, 12, 5), "200 rows: the column scans' longest run; twelve blobs")
    add("wide_1x3x4096", "largest", functools.partial(_wide, 3, 4096, (0, 2047, 2048, 4095)), "128 blocks; the first width outside the exactness domain")
    add("wide_1x2x4097", "beyond", functools.partial(_wide, 2, 4097, (5, 4096)), "a ragged 129th block; squares of gaps above 4096 round")
    add("wide_1x3x8192", "beyond", functools.partial(_wide, 3, 8192, (3, 4100, 8191)), "the widest accepted row: 33.8 KB of LDS, rounded squares and sums")
    add("lone_feature", "lone", _lone_feature, "one foreground pixel at column 0, 31, 32, 63, W - 1 and alone in the ragged last block")
    add("equal_reach", "equal_reach", _equal_reach, "two features equally far left and right, in different blocks; and one column apart")
    add("near_tradeoff", "near_tradeoff", _near_tradeoff, "g = k in the own column against g = 0 exactly k - 1, k, k + 1 columns away: gap^2 == best")
    add("empty_cols", "empty_cols", _empty_cols, "whole blocks of columns without a feature (1e9 -> 1e18) between blocks that have some")
    add("break_left", "break_left", functools.partial(_break, True), "x in block 0, the only feature in the last block: the left side is out of range from the start")
    add("break_right", "break_right", functools.partial(_break, False), "the mirror: x in the last block, the only feature in block 0")
    add("complement", "complement", _complement, "a single background pixel in a full sample and a single foreground pixel: the two passes swap roles")
    add("n3_extents", "n3_extents", _n3_extents, "a far corner pixel, a dense and an empty sample, H = 5: rows of three samples in neighbouring workgroups (row / H)")
    add("all_foreground", "all_foreground", _all_foreground, "a sample of nothing but foreground (-1 everywhere; the reference is NaN) next to an ordinary one")
    add("soft_values", "soft", _soft_values, "0.5, 0.99, 1.0, 1.5, 254.9, a denormal, -0.0; an all-soft sample; values over [0, 256)")
    add("soft_halo", "soft", _soft_halo, "a halo of 0.5 one pixel wide round a {0, 1} crack")
    add("seeded_sparse", "seeded", _seeded_sparse, "two synthetic crack masks at 96 x 200, the second bilinearly resampled to soft values")
    add("full_sparse", "full_sparse", _full_sparse, "64 x 1792 with about 0.4 % foreground: the bench's width and sparsity")
    assert len({r["name"] for r in rows}) == len(rows)
    return rows


ROWS = _table()
CLASSES = ("width", "largest", "beyond", "lone", "equal_reach", "near_tradeoff", "empty_cols", "break_left", "break_right", "complement",
           "n3_extents", "all_foreground", "soft", "seeded", "full_sparse")


def row(name):
    return next(r for r in ROWS if r["name"] == name)


@functools.lru_cache(maxsize=None)
def mask_of(name):
    m = np.ascontiguousarray(row(name)["build"](), f32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def refs(name):
    """(sdf_restated32, sdf_ref64, all-foreground samples) of a row, computed once"""
    m = mask_of(name)
    out = sdf_restated32(m), sdf_ref64(m), all_foreground(m)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def weight_refs(name):
    """(foreground, float64 distance to the nearest foreground pixel, samples without foreground, amp) of a row"""
    m = mask_of(name)
    fg, d = CW.foreground(m), CW.distance(m)
    return fg, d, ~fg.reshape(fg.shape[0], -1).any(1), weight_amp(name)


def weight_amp(name):
    """The row's amp: 80 / (the image's diagonal), rounded to float32, at most 2.  amp d <= 80 keeps every weight above
    2 exp(-80) = 3.6e-35 > FLT_MIN.  With it an error of 1 in d2 changes the weight by the factor exp(-amp (sqrt(d2 + 1) - sqrt(d2))),
    a relative change of about amp / (2 d), against the bound (amp d + 2) 2^-23: visible while amp / (2 d) > amp d 2^-23 + 2^-22, which
    holds for d2 <= D2_RESOLVED = 2^21 (amp / (2 d) >= 2 amp d 2^-23 there, and the remaining amp d 2^-23 exceeds 2^-22 for d >= 2 at
    every diagonal of the table; d = 1 is checked numerically like the rest).  Beyond d = 2048 float32 itself no longer resolves d2 + 1."""
    r = row(name)
    return float(f32(min(2.0, 80.0 / float(np.hypot(r["H"], r["W"])))))


# ------------------------------------------------------------------------------------------- comparisons (CPU mutants and the GPU test)

def bits(a):
    return (np.ascontiguousarray(a, f32) + f32(0)).view(np.uint32)          # + 0: the sign of a zero is not asked


def sdf_mismatches(got, name):
    """number of elements whose bits differ from sdf_restated32 (the sign of a zero aside)"""
    want = refs(name)[0]
    assert got.shape == want.shape and got.dtype == np.float32
    return int((bits(got) != bits(want)).sum())


def sdf_ratio(got, name):
    """(worst |got - sdf_ref64| / the counted bound, pixels left out): only the samples of nothing but foreground are left out"""
    _, ref, full = refs(name)
    keep = ~full
    err = np.abs(np.asarray(got, np.float64)[keep] - ref[keep])
    if err.size and not np.isfinite(err).all():
        return float("inf"), int(got[full].size)
    return (float(err.max()) / sdf_bound(row(name)["exact"]) if err.size else 0.0), int(got[full].size)


def sdf_caught(got, name):
    """does the GPU test's pair of comparisons reject ``got`` on this row"""
    r = row(name)
    return (r["exact"] and sdf_mismatches(got, name) > 0) or sdf_ratio(got, name)[0] > 1


def weight_check(w, name, lam=LAMBDA):
    """(w == lambda on every foreground pixel and every sample without foreground, worst relative error / ((amp d + 2) 2^-23) elsewhere)"""
    fg, d, none, amp = weight_refs(name)
    w = np.asarray(w)
    flat = fg | none[:, None, None, None]
    const_ok = bool((w[flat] == f32(lam)).all())
    ref = lam * np.exp(-amp * d)
    assert (ref >= CW.FLT_MIN).all()
    rel = np.abs(w.astype(np.float64) - ref)[~flat] / ref[~flat]
    bound = ((amp * d + 2) * 2.0 ** -23)[~flat]
    return const_ok, (float((rel / bound).max()) if rel.size else 0.0)


def weight_caught(w, name):
    ok, ratio = weight_check(w, name)
    return (not ok) or ratio > 1
