"""The crack topology (csrc/topology.hip, utils/estimate_metrics.skeleton_topology / component_topology_table / summarize_topology,
predict_dataset(topology=)) restated in NumPy, and the cases of tests/test_topology_cpu.py and tests/test_topology_gpu.py.

``topo_of`` is the definition by shifted planes, ``topo_brute`` the same by a double loop over the pixels with a neighbour lookup, and
``holes`` the flood fill (scipy.ndimage.label of the background, 4-connected, of the plane padded by one clear pixel) that ``loops`` must
equal.  Everything outside a plane is clear.

The kernel's workgroup owns TH x TW pixels and a lane a word of 32: the seams lie at y = 64, x = 128 and x = 32 k."""
import functools

import numpy as np

import components_cases as CC
import skeleton_cases as SC

TH, TW, WORD = 64, 128, 32                                # csrc/topology.hip: TP_TH, 32 * TP_TWW, bits of a word
SHAPE = SC.SHAPE                                          # 70 x 133
SHAPES = ((1, 1), (1, 12), (12, 1), (5, 7), (64, 128), (65, 129), (130, 260))
DENSITIES = (0.05, 0.3, 0.6, 0.95)
CRACK_SEEDS = (0, 1, 2)
COLUMNS = ("V", "isolated", "end", "path", "junction_px", "h", "v", "d_se", "d_sw", "q4")
ROW_COLUMNS = ("plane", "label", "end", "junction_px", "h", "v", "d_se", "d_sw", "q4", "isolated", "junctions")
RING = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))          # N, NE, E, SE, S, SW, W, NW
ISOLATED, END, PATH, JUNCTION = 1, 2, 3, 4
QUAD, LINK_E, LINK_S, LINK_SE, LINK_SW = 8, 16, 32, 64, 128
SQRT2 = 2.0 ** 0.5


# ------------------------------------------------------------------------------------------------------------ the definition
def _shift(a, dy, dx):
    """b[y, x] = a[y + dy, x + dx], clear outside the plane"""
    H, W = a.shape
    p = np.pad(a, 1)
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def topo_of(plane):
    """uint8 [H, W]: bits 0-2 the class, bit 3 the full quad, bits 4 .. 7 the owned E, S, SE, SW link"""
    s = np.asarray(plane) != 0
    r = [_shift(s, dy, dx) for dy, dx in RING]
    n8 = sum(k.astype(np.int64) for k in r)
    A = sum((~r[i] & r[(i + 1) % 8]).astype(np.int64) for i in range(8))
    cls = np.where(n8 == 0, ISOLATED, np.where(A == 1, END, np.where(A >= 3, JUNCTION, PATH)))
    n, ne, e, se, so, sw, w, nw = r
    out = np.where(s, cls, 0)
    out = out | QUAD * (s & e & so & se) | LINK_E * (s & e) | LINK_S * (s & so) | LINK_SE * (s & se & ~e & ~so) | LINK_SW * (s & sw & ~w & ~so)
    return out.astype(np.uint8)


def topo_brute(plane):
    """the same, pixel by pixel"""
    s = np.asarray(plane) != 0
    H, W = s.shape
    at = lambda y, x: bool(0 <= y < H and 0 <= x < W and s[y, x])
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if not s[y, x]:
                continue
            ring = [at(y + dy, x + dx) for dy, dx in RING]
            n8 = sum(ring)
            A = sum(1 for i in range(8) if not ring[i] and ring[(i + 1) % 8])
            v = ISOLATED if n8 == 0 else END if A == 1 else JUNCTION if A >= 3 else PATH
            if at(y, x + 1) and at(y + 1, x) and at(y + 1, x + 1):
                v |= QUAD
            if at(y, x + 1):
                v |= LINK_E
            if at(y + 1, x):
                v |= LINK_S
            if at(y + 1, x + 1) and not at(y, x + 1) and not at(y + 1, x):
                v |= LINK_SE
            if at(y + 1, x - 1) and not at(y, x - 1) and not at(y + 1, x):
                v |= LINK_SW
            out[y, x] = v
    return out


def adder_form(plane):
    """the class planes the way the kernel forms them: the eight ring terms through a bit-sliced adder (two full adders and a half adder
    for the ones, then the carries), A == 1 and A >= 3 read from the three sum planes -- (isolated, end, path, junction) bool planes"""
    s = np.asarray(plane) != 0
    r = [_shift(s, dy, dx) for dy, dx in RING]
    t = [~r[i] & r[(i + 1) % 8] for i in range(8)]
    full = lambda a, b, c: (a ^ b ^ c, (a & b) | (c & (a ^ b)))
    s0, c0 = full(t[0], t[1], t[2])
    s1, c1 = full(t[3], t[4], t[5])
    s2, c2 = t[6] ^ t[7], t[6] & t[7]
    a1, c3 = full(s0, s1, s2)
    x2, f0 = full(c0, c1, c2)
    a2, a4 = x2 ^ c3, f0 | (x2 & c3)
    any8 = functools.reduce(np.logical_or, r)
    iso, end, jun = s & ~any8, s & a1 & ~a2 & ~a4, s & ((a1 & a2) | a4)
    return iso, end, s & ~(iso | end | jun), jun


def counts_of(topo):
    """int32 [10] of one plane's topo: V, isolated, end, path, junction_px, h, v, d_se, d_sw, q4"""
    t = np.asarray(topo)
    c = t & 7
    return np.array([(c != 0).sum(), (c == ISOLATED).sum(), (c == END).sum(), (c == PATH).sum(), (c == JUNCTION).sum(), ((t & LINK_E) != 0).sum(),
                     ((t & LINK_S) != 0).sum(), ((t & LINK_SE) != 0).sum(), ((t & LINK_SW) != 0).sum(), ((t & QUAD) != 0).sum()], np.int32)


def topology_of(planes):
    """(topo uint8 [N, H, W], counts int32 [N, 10]) of a stack of planes"""
    topo = np.stack([topo_of(p) for p in planes])
    return topo, np.stack([counts_of(t) for t in topo])


def euler(counts):
    V, _, _, _, _, h, v, dse, dsw, q4 = (int(k) for k in counts)
    return V - (h + v + dse + dsw) + q4


def holes(plane):
    """the enclosed cells: the 4-connected background components that do not reach the border of the plane padded by one clear pixel"""
    from scipy.ndimage import label
    return int(label(~np.pad(np.asarray(plane) != 0, 1))[1]) - 1


def loops_of(plane, counts=None):
    """components - chi"""
    return SC.components(plane) - euler(counts_of(topo_of(plane)) if counts is None else counts)


def junctions_of(plane):
    """the 8-connected clusters of junction pixels"""
    return SC.components((topo_of(plane) & 7) == JUNCTION)


def length(h, v, dse, dsw):
    return h + v + SQRT2 * (dse + dsw)


def shares(h, v, dse, dsw):
    n = length(h, v, dse, dsw)
    return (h / n, v / n, SQRT2 * dse / n, SQRT2 * dsw / n) if n > 0 else (0.0, 0.0, 0.0, 0.0)


def summary(plane):
    """the figures of summarize_topology / predict_dataset(topology=True) of one plane, in plain Python"""
    c = [int(k) for k in counts_of(topo_of(plane))]
    links = tuple(c[5:9])
    return dict(endpoints=c[2], junctions=junctions_of(plane), junction_px=c[4], isolated_px=c[1], loops=SC.components(plane) - euler(c),
                links=links, length_geodesic_px=length(*links), orientation=shares(*links))


def link_graph_components(plane):
    """the connected components of the graph whose nodes are the set pixels and whose edges the owned links (a union-find)"""
    t = topo_of(plane)
    H, W = t.shape
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for y, x in np.argwhere(t != 0):
        for bit, dy, dx in ((LINK_E, 0, 1), (LINK_S, 1, 0), (LINK_SE, 1, 1), (LINK_SW, 1, -1)):
            if t[y, x] & bit:
                a, b = find(y * W + x), find((y + dy) * W + x + dx)
                parent[max(a, b)] = min(a, b)
    return len({find(y * W + x) for y, x in np.argwhere(t != 0)})


def topology_rows(labels, topo, min_px=1):
    """int32 [M, 11] = (plane, label, end, junction_px, h, v, d_se, d_sw, q4, isolated, junctions) per component of at least min_px pixels,
    sorted by (plane, label): the sums over the component's pixels; junctions counts the first pixels of the 8-connected junction clusters"""
    labels, topo = np.asarray(labels), np.asarray(topo)
    N, H, W = labels.shape
    rows = []
    for n in range(N):
        flat, t = labels[n].ravel().astype(np.int64), topo[n].ravel()
        c = t & 7
        jl = CC.canonical_labels((topo[n] & 7) == JUNCTION).ravel()
        marks = (c == END, c == JUNCTION, (t & LINK_E) != 0, (t & LINK_S) != 0, (t & LINK_SE) != 0, (t & LINK_SW) != 0, (t & QUAD) != 0,
                 c == ISOLATED, jl == np.arange(1, H * W + 1))
        sums = [np.bincount(flat, weights=m & (flat > 0), minlength=H * W + 1).astype(np.int64) for m in marks]
        area = np.bincount(flat, minlength=H * W + 1)
        for lab in np.nonzero(area[1:])[0] + 1:
            if area[lab] >= min_px:
                rows.append([n, lab] + [s[lab] for s in sums])
    return np.array(rows, np.int32).reshape(-1, 11)


def crack_of(sums, length_px):
    """the topology keys of one crack of predict_dataset from a row's nine sums, in plain Python"""
    end, _, h, v, dse, dsw, q4, _, junctions = (int(k) for k in sums)
    chi = length_px - (h + v + dse + dsw) + q4
    return dict(endpoints=end, junctions=junctions, loops=(1 if length_px else 0) - chi, links=(h, v, dse, dsw), length_geodesic_px=length(h, v, dse, dsw),
                orientation=shares(h, v, dse, dsw))


# ------------------------------------------------------------------------------------------------------------ shapes
def _pts(shape, pts):
    img = np.zeros(shape, np.uint8)
    for y, x in pts:
        img[y, x] = 1
    return img


def plus(arm=2):
    return [(0, d) for d in range(-arm, arm + 1)] + [(d, 0) for d in range(-arm, arm + 1) if d]


def diagonal(n=7, anti=False):
    return [(d, -d if anti else d) for d in range(-(n // 2), n - n // 2)]


def at(pts, y, x):
    return [(y + dy, x + dx) for dy, dx in pts]


# name -> (points in a 9 x 11 plane, the hand-derived values)
HAND = {
    "run7": ([(4, x) for x in range(2, 9)], dict(end=2, junction_px=0, h=6, v=0, d_se=0, d_sw=0, loops=0, length=6.0)),
    "diag7": (at(diagonal(7), 4, 5), dict(end=2, junction_px=0, h=0, v=0, d_se=6, d_sw=0, loops=0, length=6 * SQRT2)),
    "anti7": (at(diagonal(7, True), 4, 5), dict(end=2, junction_px=0, h=0, v=0, d_se=0, d_sw=6, loops=0, length=6 * SQRT2)),
    "plus": (at(plus(), 4, 5), dict(end=4, junction_px=1, loops=0, h=4, v=4)),
    "T": ([(2, x) for x in range(3, 8)] + [(3, 5), (4, 5)], dict(end=3, junction_px=1, loops=0, h=4, v=2, d_se=0, d_sw=0)),
    "square": ([(y, x) for y in range(2, 7) for x in range(3, 8) if y in (2, 6) or x in (3, 7)], dict(end=0, junction_px=0, loops=1, h=8, v=8)),
    "diamond": (at([(-2, 0), (-1, -1), (-1, 1), (0, -2), (0, 2), (1, -1), (1, 1), (2, 0)], 4, 5),
                dict(V=8, h=0, v=0, d_se=4, d_sw=4, q4=0, loops=1, end=0)),
    "L": ([(3, 4), (4, 4), (4, 5)], dict(end=2, junction_px=0, h=1, v=1, d_se=0, d_sw=0, loops=0)),
    "block": ([(3, 4), (3, 5), (4, 4), (4, 5)], dict(q4=1, loops=0, h=2, v=2, d_se=0, d_sw=0)),
    "single": ([(4, 5)], dict(V=1, isolated=1, end=0, junction_px=0, loops=0, length=0.0)),
}
HAND_SHAPE = (9, 11)


def hand(name):
    return _pts(HAND_SHAPE, HAND[name][0])


def seams():
    """uint8 [4, 70, 133]: pluses, diagonals and anti-diagonals centred on both sides of the row seam 63 / 64, the column seam 127 / 128 and
    the word seam 31 / 32, one of each on the corner where four tiles meet, and a wide plus on that corner"""
    H, W = SHAPE
    out = []
    for shape in (plus(), diagonal(7), diagonal(7, True)):
        pts = []
        for y, x in ((63, 10), (64, 20), (10, 127), (20, 128), (30, 31), (40, 32), (63, 127 - 16), (64, 128 - 8), (50, 127), (63, 50), (64, 31),
                     (63, 96), (64, 64), (63, 127)):
            pts += at(shape, y, x)
        out.append(_pts(SHAPE, pts))
    return np.stack(out + [_pts(SHAPE, at(plus(3), 64, 128))])


def borders():
    """uint8 [4, 70, 133]: runs along the first and last row, along the first and last column, the full frame, and the frame with a cross"""
    H, W = SHAPE
    a, b, c = (np.zeros(SHAPE, np.uint8) for _ in range(3))
    a[0, 3:W - 2] = a[H - 1, :] = 1
    b[2:H - 3, 0] = b[:, W - 1] = 1
    c[0] = c[H - 1] = c[:, 0] = c[:, W - 1] = 1
    d = c.copy()
    d[63] = d[:, 128] = 1
    return np.stack([a, b, c, d])


def noise(density, shape=SHAPE, seed=11):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def framed_batch():
    """uint8 [5, 13, 37]: five planes whose borders are full -- the last row of a plane and the first row of the next are both set --, noise
    inside; the values are not 0 / 1 but any non-zero byte"""
    rng = np.random.default_rng(5)
    x = (rng.random((5, 13, 37)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (5, 13, 37)).astype(np.uint8)
    x[:, 0] = x[:, -1] = x[:, :, 0] = x[:, :, -1] = 255
    return x


@functools.lru_cache(maxsize=None)
def crack_region(seed):
    return SC.random_walk_cracks(seed, *SHAPE)


@functools.lru_cache(maxsize=None)
def crack_skeleton(seed):
    return SC.skeleton(crack_region(seed)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def two_and_one():
    """(region bool [70, 133], skeleton uint8): two cracks inside the first tile and one that spans all four tiles"""
    yy, xx = np.mgrid[:SHAPE[0], :SHAPE[1]]
    region = (np.abs(yy - 10) <= 1) & (xx >= 5) & (xx <= 60)                        # a bar
    region |= (np.abs((yy - 30) - (xx - 20)) <= 1) & (yy >= 25) & (yy <= 50)        # a diagonal stroke
    region |= (np.abs((yy - 64) * 2 - (xx - 128)) <= 3) & (xx >= 70)                # through the corner of the four tiles
    region |= (np.abs(yy - 66) <= 1) & (xx >= 90)                                   # a branch of it
    return region, SC.skeleton(region).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> uint8 [N, H, W]"""
    out = {f"hand_{k}": hand(k)[None] for k in HAND}
    out["seams"] = seams()
    out["borders"] = borders()
    for d in DENSITIES:
        out[f"noise_{d}"] = noise(d)[None]
    for h, w in SHAPES:
        out[f"ones_{h}x{w}"] = np.ones((1, h, w), np.uint8)
        out[f"zeros_{h}x{w}"] = np.zeros((1, h, w), np.uint8)
        out[f"noise_{h}x{w}"] = np.stack([noise(0.3, (h, w), 3), noise(0.6, (h, w), 4)])
    out["ones"] = np.ones((1,) + SHAPE, np.uint8)
    out["zeros"] = np.zeros((1,) + SHAPE, np.uint8)
    out["framed_batch"] = framed_batch()
    out["cracks"] = np.stack([crack_skeleton(s) for s in CRACK_SEEDS])
    out["two_and_one"] = two_and_one()[1][None]
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(topo, counts) of a case, computed once"""
    return topology_of(cases()[name])


def rasterised_line(angle_deg, n=400):
    """bool plane with the 8-connected digital line (one pixel per step of the longer axis) from the origin at ``angle_deg`` in [0, 45],
    and its Euclidean length between the first and the last pixel centre"""
    t = np.tan(np.deg2rad(angle_deg))
    xs = np.arange(n + 1)
    ys = np.floor(xs * t + 0.5).astype(int)
    img = np.zeros((ys.max() + 1, n + 1), bool)
    img[ys, xs] = True
    return img, float(np.hypot(xs[-1] - xs[0], ys[-1] - ys[0]))
