"""The crack branches (csrc/branches.hip, utils/estimate_metrics.label_branches / branch_table / branch_kind / summarize_branches,
predict_dataset(branches=)) restated in NumPy, and the cases of tests/test_branches_cpu.py and tests/test_branches_gpu.py.

A branch pixel is a set pixel of class 1, 2 or 3 of ``topology_cases.topo_of``, a junction pixel one of class 4.  An owned link (bits 4 .. 7)
is INNER when both ends are branch pixels, ATTACH when exactly one end is a junction pixel, CLUSTER when both are.  ``blabels_of`` is the
definition -- the connected components of the inner links (scipy.sparse.csgraph), relabelled to 1 + the first index --, ``flood`` the same by
a flood over the links, ``kernel_form`` the same the way the kernel forms it: a union-find per tile of TH x TW pixels over the links that
stay inside the tile, then the links that cross a seam.  ``rows_of`` is the branch table by plain loops over the links and pixels."""
import functools

import numpy as np

import components_cases as CC
import topology_cases as TC

TH, TW = 64, 128                                          # csrc/branches.hip: BR_TH, 32 * BR_TWW
COLUMNS = ("plane", "label", "crack", "px", "end", "isolated", "attach", "h", "v", "d_se", "d_sw", "node_a", "node_b", "y0", "x0", "y1", "x1")
WIDTH_COLUMNS = ("max_d2", "min_d2")
KINDS = ("isolated", "free", "ring", "terminal", "self_loop", "link")
ACC = ("px", "end", "attach", "h", "v", "d_se", "d_sw", "node_a", "node_b", "x0", "y1", "x1", "max_d2", "min_d2")      # the slots of bacc
LINKS = ((TC.LINK_E, 0, 1), (TC.LINK_S, 1, 0), (TC.LINK_SE, 1, 1), (TC.LINK_SW, 1, -1))                              # bit, dy, dx: kinds 0 .. 3
BRANCH_COUNTS = {0: 77, 1: 79, 2: 88}                     # the branches of topology_cases.crack_skeleton(seed)
PARTITIONS = {0: (469, 147, 12), 1: (738, 146, 14), 2: (583, 168, 25)}      # their inner, attach and cluster links


# ------------------------------------------------------------------------------------------------------------ the definition
def is_branch(topo):
    c = np.asarray(topo) & 7
    return (c >= 1) & (c <= 3)


def is_junction(topo):
    return (np.asarray(topo) & 7) == TC.JUNCTION


def links_of(topo):
    """every owned link of one plane's topo as (p, q, kind): linear indices of the owner and of the other end, kind 0 .. 3 = E, S, SE, SW"""
    t = np.asarray(topo)
    H, W = t.shape
    out = []
    for y, x in np.argwhere(t != 0):
        for k, (bit, dy, dx) in enumerate(LINKS):
            if t[y, x] & bit:
                assert 0 <= y + dy < H and 0 <= x + dx < W and t[y + dy, x + dx] != 0, "a link of topo_of ends at a set pixel of the plane"
                out.append((int(y * W + x), int((y + dy) * W + x + dx), k))
    return out


def partition(topo):
    """(inner, attach, cluster): the links of one plane's topo by the number of junction ends, as three lists of (p, q, kind)"""
    j = is_junction(topo).ravel()
    parts = ([], [], [])
    for p, q, k in links_of(topo):
        parts[int(j[p]) + int(j[q])].append((p, q, k))
    return parts


def _first_index_labels(flat_ids, mask):
    """int32 [H W]: 1 + the smallest index of the pixels that share an id, 0 outside the mask"""
    out = np.zeros(mask.size, np.int32)
    first = {}
    for i in np.nonzero(mask)[0]:
        first.setdefault(flat_ids[i], i)
        out[i] = first[flat_ids[i]] + 1
    return out


def blabels_of(topo):
    """int32 [H, W]: 0 at clear and junction pixels, else 1 + the smallest linear index of the pixel's branch"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t = np.asarray(topo)
    H, W = t.shape
    inner = partition(t)[0]
    a = np.array([p for p, _, _ in inner], np.int64)
    b = np.array([q for _, q, _ in inner], np.int64)
    g = coo_matrix((np.ones(len(inner), np.int8), (a, b)), shape=(H * W, H * W))
    ids = connected_components(g, directed=False)[1]
    return _first_index_labels(ids, is_branch(t).ravel()).reshape(H, W)


def flood(topo):
    """the same by a flood over the inner links from every unlabelled branch pixel in raster order"""
    t = np.asarray(topo)
    H, W = t.shape
    nb = {}
    for p, q, _ in partition(t)[0]:
        nb.setdefault(p, []).append(q)
        nb.setdefault(q, []).append(p)
    out = np.zeros(H * W, np.int32)
    for s in np.nonzero(is_branch(t).ravel())[0]:
        if out[s]:
            continue
        out[s] = s + 1
        stack = [int(s)]
        while stack:
            for q in nb.get(stack.pop(), ()):
                if not out[q]:
                    out[q] = s + 1
                    stack.append(q)
    return out.reshape(H, W)


def kernel_form(topo, th=TH, tw=TW):
    """the same the way the kernel forms it: per tile a union-find over the inner links with both ends in the tile, every branch pixel then
    holding the global index of its tile-local root; the links that cross a seam joined by the smaller root; a flatten"""
    t = np.asarray(topo)
    H, W = t.shape
    inner = partition(t)[0]
    tile = lambda p: (p // W // th, p % W // tw)
    work = np.where(is_branch(t).ravel(), np.arange(H * W), -1)

    def find(i):
        while work[i] < i:
            i = work[i]
        return i

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            work[max(a, b)] = min(a, b)

    for p, q, _ in inner:
        if tile(p) == tile(q):
            union(p, q)
    for i in np.nonzero(work >= 0)[0]:                    # the local pass ends flat: the tile-local root
        work[i] = find(i)
        assert tile(work[i]) == tile(i)
    seam = [(p, q, k) for p, q, k in inner if tile(p) != tile(q)]
    for p, q, k in seam:                                  # only E, SE from a last column, SW from a first column, S, SE, SW from a last row
        y, x = divmod(p, W)
        assert (y % th == th - 1 and k in (1, 2, 3)) or (x % tw == tw - 1 and k in (0, 2)) or (x % tw == 0 and k == 3)
        union(p, q)
    return np.array([find(i) + 1 if work[i] >= 0 else 0 for i in range(H * W)], np.int32).reshape(H, W), len(seam)


# ------------------------------------------------------------------------------------------------------------ the sums
def sums_of(topo, blabels, jlabels=None, d2=None):
    """{label: dict over ACC} of one plane, by plain loops: the pixels first, then every inner and attach link"""
    t, bl = np.asarray(topo), np.asarray(blabels)
    H, W = t.shape
    jl = None if jlabels is None else np.asarray(jlabels).ravel()
    out = {}
    for y, x in np.argwhere(bl != 0):
        a = out.setdefault(int(bl[y, x]), dict(px=0, end=0, attach=0, h=0, v=0, d_se=0, d_sw=0, node_a=0, node_b=0, x0=W, y1=0, x1=0, max_d2=0, min_d2=0))
        a["px"] += 1
        a["end"] += int((t[y, x] & 7) == TC.END)
        a["x0"], a["y1"], a["x1"] = min(a["x0"], int(x)), max(a["y1"], int(y)), max(a["x1"], int(x))
        if d2 is not None and d2[y, x] > 0:
            v = int(d2[y, x])
            a["max_d2"] = max(a["max_d2"], v)
            a["min_d2"] = v if a["min_d2"] == 0 else min(a["min_d2"], v)
    flat = bl.ravel()
    inner, attach, _ = partition(t)
    for p, q, k in inner:
        assert flat[p] == flat[q] != 0
        out[int(flat[p])][ACC[3 + k]] += 1
    for p, q, k in attach:
        b, j = (p, q) if flat[p] != 0 else (q, p)          # the branch end and the junction end, whichever owns the link
        assert flat[b] != 0 and flat[j] == 0
        a = out[int(flat[b])]
        a[ACC[3 + k]] += 1
        a["attach"] += 1
        if jl is not None:
            v = int(jl[j])
            assert v > 0
            a["node_a"] = v if a["node_a"] == 0 else min(a["node_a"], v)
            a["node_b"] = max(a["node_b"], v)
    return out


def junction_labels(topo):
    """int32 [H, W]: the 8-connected clusters of the junction pixels, labelled 1 + first index"""
    return CC.canonical_labels(is_junction(topo))


def rows_of(topo, jlabels=True, labels=None, d2=None, blabels=None):
    """int32 [M, 17 or 19] = COLUMNS (+ WIDTH_COLUMNS with d2) for topo uint8 [N, H, W], sorted by (plane, label).  ``jlabels`` True: the
    junction clusters of the plane; None: none; ``labels`` / ``d2`` int [N, H, W] or None"""
    topo = np.asarray(topo)
    N, H, W = topo.shape
    rows = []
    for n in range(N):
        bl = blabels_of(topo[n]) if blabels is None else np.asarray(blabels[n])
        jl = junction_labels(topo[n]) if jlabels is True else None if jlabels is None else np.asarray(jlabels[n])
        sums = sums_of(topo[n], bl, jl, None if d2 is None else np.asarray(d2[n]))
        for lab in sorted(sums):
            a, (y, x) = sums[lab], divmod(lab - 1, W)
            row = [n, lab, 0 if labels is None else int(labels[n][y, x]), a["px"], a["end"], int((topo[n][y, x] & 7) == TC.ISOLATED), a["attach"], a["h"],
                   a["v"], a["d_se"], a["d_sw"], a["node_a"], a["node_b"], y, a["x0"], a["y1"], a["x1"]]
            rows.append(row + ([a["max_d2"], a["min_d2"]] if d2 is not None else []))
    return np.array(rows, np.int32).reshape(-1, len(COLUMNS) + (2 if d2 is not None else 0))


def bacc_of(topo, blabels, jlabels=None, d2=None, fill=0):
    """int32 [N, 12 or 14, H W] the way csbsr_branch_sums leaves it: the sums at the root slots, ``fill`` everywhere else"""
    topo = np.asarray(topo)
    N, H, W = topo.shape
    K = 12 if d2 is None else 14
    out = np.full((N, K, H * W), fill, np.int32)
    for n in range(N):
        sums = sums_of(topo[n], blabels[n], None if jlabels is None else jlabels[n], None if d2 is None else d2[n])
        for lab, a in sums.items():
            out[n, :, lab - 1] = [a[k] for k in ACC[:K]]
    return out


def kind_of(end, attach, node_a, node_b, isolated):
    """the truth table of the branch kinds, read top to bottom"""
    if isolated:
        return "isolated"
    if attach == 0 and end == 2:
        return "free"
    if attach == 0 and end == 0:
        return "ring"
    if end >= 1 and attach >= 1:
        return "terminal"
    if end == 0 and attach >= 1 and node_a == node_b:
        return "self_loop"
    return "link"


def kinds_of(rows):
    c = {k: j for j, k in enumerate(COLUMNS)}
    return [kind_of(r[c["end"]], r[c["attach"]], r[c["node_a"]], r[c["node_b"]], r[c["isolated"]]) for r in np.asarray(rows).tolist()]


def branch_dicts(rows, W, crack_of_label=None):
    """the ``branches`` list of predict_dataset from the rows of one plane, in plain Python"""
    c = {k: j for j, k in enumerate(COLUMNS)}
    out = []
    for r, kind in zip(np.asarray(rows).tolist(), kinds_of(rows)):
        links = (r[c["h"]], r[c["v"]], r[c["d_se"]], r[c["d_sw"]])
        y, x = divmod(r[c["label"]] - 1, W)
        d = dict(y=y, x=x, kind=kind, px=r[c["px"]], ends=r[c["end"]], attach=r[c["attach"]], nodes=(r[c["node_a"]], r[c["node_b"]]), links=links,
                 length_geodesic_px=TC.length(*links), orientation=TC.shares(*links), bbox=(r[c["y0"]], r[c["x0"]], r[c["y1"]], r[c["x1"]]))
        if crack_of_label is not None:
            d["crack"] = crack_of_label[r[c["crack"]]]
        if len(r) > len(COLUMNS):
            d.update(max_width_px=width_of_d2(r[len(COLUMNS)]), min_width_px=width_of_d2(r[len(COLUMNS) + 1]))
        out.append(d)
    return out


def width_of_d2(d2):
    """the local width of a squared distance: 2 sqrt(d2) - 1, 0.0 for 0"""
    return float(2.0 * np.sqrt(np.float64(d2)) - 1.0) if d2 > 0 else 0.0


# ------------------------------------------------------------------------------------------------------------ shapes
_DIAMOND = [(-2, 0), (-1, -1), (-1, 1), (0, -2), (0, 2), (1, -1), (1, 1), (2, 0)]
# name -> (points in a 9 x 11 plane, the branches, the sorted kinds, the junction pixels)
HAND = {
    "T": (TC.HAND["T"][0], 3, ["terminal"] * 3, 1),
    "plus": (TC.HAND["plus"][0], 4, ["terminal"] * 4, 1),
    "Y": ([(4, 5), (5, 5), (6, 5), (3, 4), (2, 3), (3, 6), (2, 7)], 3, ["terminal"] * 3, 1),
    "ring": (TC.HAND["square"][0], 1, ["ring"], 0),
    "diamond": (TC.HAND["diamond"][0], 1, ["ring"], 0),
    "eight": (TC.at(_DIAMOND, 4, 3) + TC.at(_DIAMOND, 4, 7), 2, ["self_loop"] * 2, 1),
    "theta": ([(y, x) for y in range(1, 8) for x in range(1, 10) if y in (1, 7) or x in (1, 5, 9)], 3, ["link"] * 3, 2),
    "run7": (TC.HAND["run7"][0], 1, ["free"], 0),
    "single": (TC.HAND["single"][0], 1, ["isolated"], 0),
    "two_singles": ([(1, 1), (6, 8)], 2, ["isolated"] * 2, 0),
}


def hand(name):
    return TC._pts(TC.HAND_SHAPE, HAND[name][0])


def corner_strokes():
    """uint8 [2, 70, 133]: diagonal and anti-diagonal strokes through and beside the corner where four tiles meet, so that SE and SW links
    cross the row seam, the column seam and the corner itself; the second plane adds crossing strokes, whose crossings are junctions"""
    H, W = TC.SHAPE
    a = np.zeros(TC.SHAPE, np.uint8)

    def stroke(img, y, x, sx, n=6):
        for d in range(-n, n + 1):
            if 0 <= y + d < H and 0 <= x + sx * d < W:
                img[y + d, x + sx * d] = 1

    for y, x in ((64, 128), (63, 120), (60, 127), (50, 128), (64, 100), (66, 127)):
        stroke(a, y, x, 1)
    for y, x in ((63, 40), (40, 128), (63, 90)):
        stroke(a, y, x, -1)
    b = a.copy()
    stroke(b, 64, 127, -1)                                                           # the anti-diagonal through the corner
    stroke(b, 30, 127, -1)                                                           # an X over the column seam
    stroke(b, 30, 128, 1)
    return np.stack([a, b])


def seam_T():
    """uint8 [3, 70, 133]: a T whose junction pixel lies on a seam and whose arms lie in three tiles -- the bar along the last row of the
    upper tiles with the stem below the corner; the bar down the last column of the left tiles with the stem to the right; and a T whose
    junction is the first pixel of the fourth tile"""
    a, b, c = (np.zeros(TC.SHAPE, np.uint8) for _ in range(3))
    a[63, 120:133] = 1
    a[64:70, 127] = 1
    b[55:70, 127] = 1
    b[63, 128:133] = 1
    c[64, 120:133] = 1
    c[58:64, 128] = 1
    return np.stack([a, b, c])


def ones_between_zeros():
    """uint8 [5, 13, 37]: a plane of ones between planes of zeros"""
    x = np.zeros((5, 13, 37), np.uint8)
    x[2] = 1
    return x


@functools.lru_cache(maxsize=None)
def cases():
    """name -> uint8 [N, H, W] planes (the skeleton, or any plane)"""
    out = {f"hand_{k}": hand(k)[None] for k in HAND}
    out["seams"] = TC.seams()
    out["borders"] = TC.borders()
    out["corner_strokes"] = corner_strokes()
    out["seam_T"] = seam_T()
    for d in TC.DENSITIES:
        out[f"noise_{d}"] = TC.noise(d)[None]
    for h, w in TC.SHAPES:
        out[f"ones_{h}x{w}"] = np.ones((1, h, w), np.uint8)
        out[f"zeros_{h}x{w}"] = np.zeros((1, h, w), np.uint8)
        out[f"noise_{h}x{w}"] = np.stack([TC.noise(0.3, (h, w), 3), TC.noise(0.6, (h, w), 4)])
    out["ones"] = np.ones((1,) + TC.SHAPE, np.uint8)
    out["zeros"] = np.zeros((1,) + TC.SHAPE, np.uint8)
    out["ones_between_zeros"] = ones_between_zeros()
    out["framed_batch"] = TC.framed_batch()
    out["cracks"] = np.stack([TC.crack_skeleton(s) for s in TC.CRACK_SEEDS])
    out["cracks_pruned"] = np.stack([pruned_crack_skeleton(s) for s in TC.CRACK_SEEDS])
    out["two_and_one"] = TC.two_and_one()[1][None]
    return out


@functools.lru_cache(maxsize=None)
def pruned_crack_skeleton(seed, spur=6):
    import prune_cases as PR
    return PR.prune(TC.crack_skeleton(seed), spur)[0].astype(np.uint8)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(topo uint8 [N, H, W], blabels int32 [N, H, W], jlabels int32 [N, H, W]) of a case, computed once"""
    topo = np.stack([TC.topo_of(p) for p in cases()[name]])
    return topo, np.stack([blabels_of(t) for t in topo]), np.stack([junction_labels(t) for t in topo])


def fake_d2(blabels, seed=9):
    """an int32 map like skeleton_width's: positive at most branch pixels, 0 at some of them and at every other pixel"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 40, size=np.shape(blabels)).astype(np.int32)
    d[rng.random(np.shape(blabels)) < 0.2] = 0
    return np.where(np.asarray(blabels) != 0, d, 0).astype(np.int32)
