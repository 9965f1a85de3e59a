"""The polyline simplification (csrc/simplify.hip, utils/estimate_metrics.simplify_polylines / simplify_tolerance / polyline_length,
predict_dataset(simplify_px=)) restated in NumPy, and the cases of tests/test_simplify_cpu.py and tests/test_simplify_gpu.py.

A table is (offsets int64 [M + 1], points int32 [P, 4]) as branch_polylines returns it; only y and x are read.  For a segment from kept point
a to kept point b and a point p strictly between them, c2 = |b - a|^2, t = (p - a).(b - a), and the KEY is |p - a|^2 if c2 = 0,
|p - a|^2 c2 if t <= 0, |p - b|^2 c2 if t >= c2, else cross(b - a, p - a)^2.  The inner point with the largest key -- the smallest row among
equals -- is kept iff 16 key > tol_q^2 c2 (c2 = 0: 16 key > tol_q^2) and splits the segment; the first and the last row are always kept.

``simplify_stack`` is the recursion with an explicit stack; ``simplify_rounds`` examines all segments of a level at once, as the kernel does,
and counts its rounds.  Both use int64 / Python integers only: with coordinates in [0, 8192) every term stays below 2^58."""
import functools

import numpy as np

import polyline_cases as PC

TOL_Q = (0, 1, 2, 4, 6, 8, 64)
ROUTE_LIMITS = (64, 2048)                                                            # estimate_metrics.SIMPLIFY_ROUTE_LIMITS, asserted by the tests
SIDE = 8192


# ------------------------------------------------------------------------------------------------------------ the definition
def keys_of(a, b, p):
    """int64 [n] keys of the points p [n, 2] against the segments a -> b ([2] or [n, 2] each), and c2 int64 (scalar or [n])"""
    a, b, p = (np.asarray(v, np.int64) for v in (a, b, p))
    dy, dx = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    ey, ex = p[..., 0] - a[..., 0], p[..., 1] - a[..., 1]
    fy, fx = p[..., 0] - b[..., 0], p[..., 1] - b[..., 1]
    c2 = dy * dy + dx * dx
    t = ey * dy + ex * dx
    pa, pb, cr = ey * ey + ex * ex, fy * fy + fx * fx, dx * ey - dy * ex
    key = np.where(c2 == 0, pa, np.where(t <= 0, pa * c2, np.where(t >= c2, pb * c2, cr * cr)))
    return key, c2


def splits(key, c2, tol_q):
    """the split rule in Python integers"""
    key, c2 = int(key), int(c2)
    return 16 * key > tol_q * tol_q * (c2 if c2 else 1)


def _yx(yx):
    """int64 [n, 2]: y and x of a span's rows"""
    a = np.asarray(yx, np.int64)
    return a.reshape(a.shape[0], -1)[:, :2] if a.size else np.zeros((0, 2), np.int64)


def simplify_stack(yx, tol_q):
    """uint8 [n] keep flags of one span's points [n, 2 or more] by the recursion, with an explicit stack"""
    yx = _yx(yx)
    n = yx.shape[0]
    keep = np.zeros(n, np.uint8)
    if n == 0:
        return keep
    keep[0] = keep[-1] = 1
    stack = [(0, n - 1)]
    while stack:
        a, b = stack.pop()
        if b - a < 2:
            continue
        key, c2 = keys_of(yx[a], yx[b], yx[a + 1:b])
        i = int(np.argmax(key))                                                      # the first of the largest: the smallest row
        if splits(key[i], c2, tol_q):
            w = a + 1 + i
            keep[w] = 1
            stack += [(a, w), (w, b)]
    return keep


def simplify_rounds(yx, tol_q):
    """(keep uint8 [n], rounds) of one span by rounds: every round examines all the segments the round before made, vectorised over their
    inner points; rounds counts the rounds that examined a segment, the last of which splits nothing"""
    yx = _yx(yx)
    n = yx.shape[0]
    keep = np.zeros(n, np.uint8)
    if n == 0:
        return keep, 0
    keep[0] = keep[-1] = 1
    A, B = np.array([0], np.int64), np.array([n - 1], np.int64)
    rounds = 0
    while True:
        some = B - A >= 2
        A, B = A[some], B[some]
        if A.size == 0:
            return keep, rounds
        rounds += 1
        inner = B - A - 1
        first = np.concatenate([np.zeros(1, np.int64), np.cumsum(inner)])[:-1]       # the segment's first inner point in the flat list
        seg = np.repeat(np.arange(A.size), inner)
        row = np.arange(int(inner.sum())) - np.repeat(first, inner) + np.repeat(A + 1, inner)
        key, c2 = keys_of(yx[A[seg]], yx[B[seg]], yx[row])
        kmax = np.maximum.reduceat(key, first)
        w = np.minimum.reduceat(np.where(key == kmax[seg], row, n), first)           # the smallest row among the equals
        c2s = c2[first]
        split = np.array([splits(k, c, tol_q) for k, c in zip(kmax.tolist(), c2s.tolist())], bool)
        keep[w[split]] = 1
        A, B = np.concatenate([A[split], w[split]]), np.concatenate([w[split], B[split]])


def simplify_table(offsets, points, tol_q, form=simplify_rounds):
    """(keep uint8 [P], vcount int32 [M]) of a table; a span whose offsets descend or leave 0 .. P is skipped, rows outside every span are 0"""
    offsets, points = np.asarray(offsets, np.int64), np.asarray(points).reshape(-1, 4)
    P, M = points.shape[0], offsets.size - 1
    keep, vcount = np.zeros(P, np.uint8), np.zeros(M, np.int32)
    for j in range(M):
        o0, o1 = int(offsets[j]), int(offsets[j + 1])
        if not 0 <= o0 <= o1 <= P:
            continue
        k = form(points[o0:o1, :2], tol_q)
        k = k[0] if isinstance(k, tuple) else k
        keep[o0:o1] |= k
        vcount[j] = int(k.sum())
    return keep, vcount


def segment_distance(a, b, p):
    """the distance of p from the segment a -> b in fp64, by projection: independent of the integer key"""
    a, b, p = (np.asarray(v, np.float64) for v in (a, b, p))
    d = b - a
    c2 = float(d @ d)
    u = 0.0 if c2 == 0 else min(1.0, max(0.0, float((p - a) @ d) / c2))
    return float(np.hypot(*(p - (a + u * d))))


# ------------------------------------------------------------------------------------------------------------ the tables
def table_of(spans):
    """(offsets, points) of a list of spans, each a list of (y, x); diag and d2 are filled with values that must not matter"""
    offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum([len(s) for s in spans])]).astype(np.int64)
    yx = np.array([p for s in spans for p in s], np.int64).reshape(-1, 2)
    assert yx.size == 0 or (yx.min() >= 0 and yx.max() < SIDE)
    points = np.concatenate([yx, np.arange(yx.shape[0])[:, None] % 7, 1000 + np.arange(yx.shape[0])[:, None]], 1).astype(np.int32)
    return offsets, points


def digital_line(num, den=50):
    """the den + 1 pixels of the digital straight line of slope num / den: x = 0 .. den, y = the nearest row"""
    return [((x * num * 2 + den) // (2 * den), x) for x in range(den + 1)]


LINE_SLOPES = (0, 7, 20, 33, 50)


def saw(n):
    """a saw whose teeth grow: every round of the simplification finds one tooth"""
    return [((i % 2) * (i + 1), 3 * i) for i in range(n)]


ZIGZAG = [(0, 0), (3, 2), (0, 4), (3, 6), (0, 8)]                                    # rows 1 and 3 have equal keys, then rows 2 and 3


def random_walk(n, seed):
    rng = np.random.default_rng(seed)
    step = rng.integers(-1, 2, size=(n, 2))
    step[(step == 0).all(1)] = (0, 1)
    yx = np.clip(4000 + np.cumsum(step, 0), 0, SIDE - 1)
    return [tuple(p) for p in yx.tolist()]


def random_points(n, seed):
    rng = np.random.default_rng(seed)
    yx = rng.integers(0, SIDE, size=(n, 2))
    for k, c in zip(rng.choice(np.arange(1, n - 1), 4, replace=False), ((0, 0), (0, SIDE - 1), (SIDE - 1, 0), (SIDE - 1, SIDE - 1))):
        yx[k] = c
    return [tuple(p) for p in yx.tolist()]


POLYLINE_NAMES = ("cracks", "noise_0.3", "noise_0.6", "corner_rings", "staircase", "borders", "zeros", "serpentine_66x130", "serpentine_130x260")


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (offsets int64 [M + 1], points int32 [P, 4])"""
    out = {}
    for name in POLYLINE_NAMES:
        topo, bl, rank, diag, _ = PC.expected(name)
        _, offsets, points = PC.polylines_of(bl, rank, diag)
        out[name] = (offsets, points)
    out["tiny_spans"] = table_of([[], [(3, 3)], [(1, 1), (5, 2)], [], [(0, 0), (4, 1), (0, 2)], [(7, 7), (7, 8), (7, 9)], []])
    out["collinear"] = table_of([[(5, x) for x in range(40)], [(y, 9) for y in range(70)], [(k, k) for k in range(30)], [(2 * k, k) for k in range(100)],
                                 [(90 - k, 3 * k) for k in range(31)]])
    out["digital_lines"] = table_of([digital_line(s) for s in LINE_SLOPES])
    out["zigzag_tie"] = table_of([ZIGZAG, [(y + 10, x) for y, x in ZIGZAG[::-1]]])
    out["saw_60"] = table_of([saw(60)])
    out["saw_1500"] = table_of([saw(1500)])
    out["random_corners"] = table_of([random_points(200, 5)])
    out["repeated_points"] = table_of([[(5, 5), (5, 9), (9, 9), (5, 5)], [(1, 1), (1, 1), (1, 1)], [(2, 2), (2, 2), (7, 7), (2, 2), (2, 2)],
                                       [(4, 4), (4, 4)], [(3, 0), (3, 5), (3, 5), (3, 5), (0, 9), (3, 5), (8, 8)]])
    out["route_seams"] = table_of([random_walk(L + d, 100 * L + d + 1) for L in ROUTE_LIMITS for d in (-1, 0, 1)])
    a, b = out["cracks"], out["route_seams"]
    for tag, (first, second) in (("ab", (a, b)), ("ba", (b, a))):
        out["swapped_" + tag] = (np.concatenate([first[0], second[0][1:] + first[0][-1]]), np.concatenate([first[1], second[1]]))
    return out


@functools.lru_cache(maxsize=None)
def expected(name, tol_q):
    """(keep uint8 [P], vcount int32 [M]) of a case by the rounds form, computed once"""
    keep, vcount = simplify_table(*cases()[name], tol_q)
    keep.setflags(write=False)
    vcount.setflags(write=False)
    return keep, vcount


def vertex_dicts(branches, tol_q, widths=False):
    """the keys predict_dataset(simplify_px=) adds to every dict of ``branches``, from the dicts' own points: (list of dicts, vertices, sum of
    the lengths); the length of a closed chain -- as many inner links as pixels -- includes the segment back to the first vertex"""
    out, nv, total = [], 0, 0.0
    for b in branches:
        pts = np.asarray(b["points"]).reshape(-1, 2)
        keep = simplify_stack(pts, tol_q)
        idx = np.nonzero(keep)[0].astype(np.int32)
        d = dict(vertices=pts[idx].astype(np.int32), vertex_index=idx, length_simplified_px=None)
        if b["chain"]:
            closed = sum(b["links"]) - b["attach"] == b["px"]
            v = [(float(y), float(x)) for y, x in pts[idx].tolist()]
            v = v + v[:1] if closed and len(v) >= 2 else v
            d["length_simplified_px"] = float(sum(np.hypot(q[0] - p[0], q[1] - p[1]) for p, q in zip(v, v[1:])))
            total += d["length_simplified_px"]
        if widths:
            d["vertex_width_px"] = np.asarray(b["width_profile_px"], np.float64)[idx]
        nv += idx.size
        out.append(d)
    return out, nv, total
