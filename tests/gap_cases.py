"""Crack gap bridging (csrc/gaps.hip, utils/estimate_metrics.endpoint_gaps / gap_table / gap_groups / draw_bridges,
predict_dataset(bridge_gap_px=)) restated in NumPy, and the cases of tests/test_gaps_cpu.py and tests/test_gaps_gpu.py.  All integers.

topo is the byte plane of ``topology_cases.topo_of`` (class = topo & 7: 0 clear, 1 isolated, 2 end, 3 path, 4 junction), labels any int32
label map.  A source is a pixel p of class 1 or 2 with labels[p] != 0; a candidate for p is a pixel q of the same plane with class != 0
(``to`` = "end": class 1 or 2), labels[q] != 0, labels[q] != labels[p] and d2 = |q - p|^2 <= G^2; the gap of p is the candidate with the
smallest 64-bit key (d2 << 32) | q, q the linear index.

The search has two independent forms: ``gaps_brute`` takes the minimum key over ALL the targets of the plane, a matrix of sources against
targets; ``gaps_window`` walks the rows around each source the way the kernel does -- dy = 0, -1, +1, ... while dy^2 <= the best so far, in
a row the set pixels within the largest |dx| that can still win -- and the CPU test holds the two equal on every case.

The kernel's workgroup owns TH x TW pixels: the seams lie at y = 64 and x = 128."""
import functools

import numpy as np

import components_cases as CC
import skeleton_cases as SC
import topology_cases as TC

TH, TW = 64, 128                                          # csrc/gaps.hip: GP_TH, GP_TW
WAVE_SRC = 32                                             # GP_WAVE_SRC: up to this many sources in a tile get a wave each, more a lane each
MAX_G = 64
SHAPE = SC.SHAPE                                          # 70 x 133
BIG = (2 * TH + 6, 2 * TW + 5)                            # 134 x 261: a whole tile between two others
GAPS = (2, 3, 5, 16, 64)
TOS = ("any", "end")
COLUMNS = ("plane", "p", "q", "d2", "label_p", "label_q", "class_q", "mutual")
CRACK_MASKS = ((2, 67, 263), (6, 131, 135), (4, 70, 133))                       # components_cases.broken_cracks(seed, H, W)
CRACK_GAPS = (2, 4, 8, 64)
# the number of "any" gaps of each mask at G = 2 / 4 / 8 / 64, from a brute-force search on these exact inputs
CRACK_COUNTS = {(2, 67, 263): (9, 32, 52, 64), (6, 131, 135): (13, 46, 71, 86), (4, 70, 133): (7, 27, 46, 53)}
NOISE_GAPS = (2, 5, 64)


# ------------------------------------------------------------------------------------------------------------ the definition
def _masks(topo, labels, to):
    cls = topo & 7
    lab = labels != 0
    src = ((cls == 1) | (cls == 2)) & lab
    tgt = (src if to == "end" else (cls != 0) & lab)
    return src, tgt


def gaps_brute(topo, labels, G, to="any"):
    """(gap_q, gap_d2) int32 [N, H, W]: the minimum of the 64-bit key over every target of the plane"""
    assert to in TOS and 2 <= G <= MAX_G
    topo, labels = np.asarray(topo), np.asarray(labels)
    N, H, W = topo.shape
    gq, gd = np.full((N, H, W), -1, np.int32), np.zeros((N, H, W), np.int32)
    none = np.int64((G * G + 1) << 32)
    for n in range(N):
        src, tgt = _masks(topo[n], labels[n], to)
        sy, sx = np.nonzero(src)
        ty, tx = np.nonzero(tgt)
        if not len(sy) or not len(ty):
            continue
        tl, tq = labels[n][ty, tx], (ty * W + tx).astype(np.int64)
        for a in range(0, len(sy), 512):
            y, x = sy[a:a + 512, None].astype(np.int64), sx[a:a + 512, None].astype(np.int64)
            d2 = (ty[None] - y) ** 2 + (tx[None] - x) ** 2
            key = np.where((d2 <= G * G) & (tl[None] != labels[n][sy[a:a + 512], sx[a:a + 512]][:, None]), (d2 << 32) | tq[None], none)
            best = key.min(1)
            has = best < none
            gq[n][sy[a:a + 512][has], sx[a:a + 512][has]] = (best[has] & 0xFFFFFFFF).astype(np.int32)
            gd[n][sy[a:a + 512][has], sx[a:a + 512][has]] = (best[has] >> 32).astype(np.int32)
    return gq, gd


def gaps_window(topo, labels, G, to="any"):
    """the same by the kernel's walk: rows outward from the source, in a row only the columns that can still win"""
    assert to in TOS and 2 <= G <= MAX_G
    topo, labels = np.asarray(topo), np.asarray(labels)
    N, H, W = topo.shape
    gq, gd = np.full((N, H, W), -1, np.int32), np.zeros((N, H, W), np.int32)
    for n in range(N):
        src, _ = _masks(topo[n], labels[n], to)
        cls = topo[n] & 7
        bits = ((cls == 1) | (cls == 2)) if to == "end" else cls != 0          # the label is looked up at a set bit only
        for py, px in zip(*(v.tolist() for v in np.nonzero(src))):
            mine = labels[n, py, px]
            lim, bq, m = G * G, -1, G
            dy = 0
            while dy * dy <= lim:
                for ry in ((0,) if dy == 0 else (-dy, dy)):
                    if dy * dy > lim:
                        break
                    while dy * dy + m * m > lim:
                        m -= 1
                    y = py + ry
                    if not 0 <= y < H:
                        continue
                    x0 = max(px - m, 0)
                    xs = np.nonzero(bits[y, x0:px + m + 1])[0] + x0
                    xs = xs[(labels[n, y, xs] != 0) & (labels[n, y, xs] != mine)]
                    if not len(xs):
                        continue
                    d = dy * dy + (xs - px) ** 2                                 # the row's own minimum of (d2, q): q grows with x
                    k = int(np.argmin(d))
                    if d[k] < lim or (d[k] == lim and (bq < 0 or y * W + xs[k] < bq)):
                        lim, bq = int(d[k]), int(y * W + xs[k])
                dy += 1
            if bq >= 0:
                gq[n, py, px], gd[n, py, px] = bq, lim
    return gq, gd


def gap_table(topo, labels, gq, gd):
    """int32 [M, 8] = COLUMNS, in raster order of p, plane by plane; mutual is gap_q[q] == p"""
    N, H, W = gq.shape
    n, y, x = np.nonzero(gq >= 0)
    p = y * W + x
    q = gq[n, y, x].astype(np.int64)
    fl, ft, fq = labels.reshape(N, -1), topo.reshape(N, -1), gq.reshape(N, -1)
    cols = [n, p, q, gd[n, y, x], fl[n, p], fl[n, q], ft[n, q] & 7, fq[n, q] == p]
    return np.stack([np.asarray(c, np.int64) for c in cols], 1).astype(np.int32).reshape(-1, 8)


def groups_of(labels, gq):
    """int32 [N, H, W]: every label replaced by the smallest label of its group (scipy's connected components of the label graph)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    labels = np.asarray(labels)
    N, H, W = labels.shape
    out = np.zeros_like(labels)
    for n in range(N):
        fl = labels[n].ravel().astype(np.int64)
        assert fl.min() >= 0 and fl.max() <= H * W
        p = np.nonzero(gq[n].ravel() >= 0)[0]
        a, b = fl[p], fl[gq[n].ravel()[p]]
        _, comp = connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(H * W + 1, H * W + 1)), directed=False)
        lowest = np.full(comp.max() + 1, H * W + 1, np.int64)
        np.minimum.at(lowest, comp, np.arange(H * W + 1))
        out[n] = np.where(labels[n] != 0, lowest[comp[fl]].reshape(H, W), 0)
    return out.astype(np.int32)


def groups_union_find(labels, gq):
    """the same with a union-find over the labels, the smaller root winning"""
    labels = np.asarray(labels)
    N, H, W = labels.shape
    out = np.zeros_like(labels)
    for n in range(N):
        parent = {}

        def find(i):
            while parent.setdefault(i, i) != i:
                i = parent[i]
            return i
        fl, fq = labels[n].ravel(), gq[n].ravel()
        for p in np.nonzero(fq >= 0)[0].tolist():
            a, b = find(int(fl[p])), find(int(fl[fq[p]]))
            if a != b:
                parent[max(a, b)] = min(a, b)
        out[n] = np.array([find(int(v)) if v else 0 for v in fl], np.int32).reshape(H, W)
    return out.astype(np.int32)


def bresenham(a, b):
    """the pixels [(y, x)] of the bridge between (y, x) pairs a and b, drawn from the one with the smaller linear index; y1 >= y0"""
    (y, x), (y1, x1) = sorted([tuple(int(v) for v in a), tuple(int(v) for v in b)])
    dx, dy, sx = abs(x1 - x), y1 - y, (x1 > x) - (x1 < x)
    err, out = dx - dy, []
    while True:
        out.append((y, x))
        if (y, x) == (y1, x1):
            return out
        e2 = 2 * err
        if e2 > -dy:
            err -= dy
            x += sx
        if e2 < dx:
            err += dx
            y += 1


def bridges_of(gq):
    """uint8 [N, H, W] of 0 / 1: the bridge of every gap"""
    N, H, W = gq.shape
    out = np.zeros((N, H, W), np.uint8)
    for n, y, x in zip(*np.nonzero(gq >= 0)):
        for yy, xx in bresenham((y, x), divmod(int(gq[n, y, x]), W)):
            out[n, yy, xx] = 1
    return out


def summary_of(rows, n_cracks):
    """the figures of ``summarize_gaps`` from the rows of one plane, by loops"""
    rows = np.asarray(rows, np.int64).reshape(-1, 8)
    length, parent = 0.0, {}

    def find(i):
        while parent.setdefault(i, i) != i:
            i = parent[i]
        return i
    merges = 0
    for _, p, q, d2, la, lb, _, mutual in rows.tolist():
        if not mutual or p < q:
            length += float(np.sqrt(np.float64(d2)))
        a, b = find(la), find(lb)
        if a != b:
            parent[max(a, b)] = min(a, b)
            merges += 1
    ee = int(np.isin(rows[:, 6], (1, 2)).sum())
    return dict(n_gaps=len(rows), n_mutual=int(rows[:, 7].sum()), n_end_to_end=ee, n_end_to_side=len(rows) - ee, gap_length_px=length,
                max_gap_px=float(np.sqrt(np.float64(rows[:, 3].max()))) if len(rows) else 0.0, n_cracks_bridged=n_cracks - merges)


# ------------------------------------------------------------------------------------------------------------ inputs
def of_skeleton(*planes, labels=None):
    """(topo uint8 [N, H, W], labels int32 [N, H, W]) of binary planes: their topo bytes and, without ``labels``, their own canonical labels"""
    sk = np.stack([np.asarray(p) != 0 for p in planes])
    topo = np.stack([TC.topo_of(p) for p in sk])
    lab = np.stack([CC.canonical_labels(p) for p in sk]) if labels is None else np.asarray(labels, np.int32).reshape(sk.shape)
    return topo, lab.astype(np.int32)


def _plane(shape, *runs):
    """a bool plane with the runs ((y0, x0), (y1, x1)) -- inclusive, axis-parallel -- and the pixels (y, x) set"""
    img = np.zeros(shape, bool)
    for r in runs:
        if isinstance(r[0], tuple):
            (y0, x0), (y1, x1) = r
            img[y0:y1 + 1, x0:x1 + 1] = True
        else:
            img[r] = True
    return img


HAND_SHAPE = (14, 24)


def collinear():
    return _plane(HAND_SHAPE, ((4, 2), (4, 8)), ((4, 12), (4, 18)))


def tee():
    return _plane(HAND_SHAPE, ((10, 2), (10, 20)), ((2, 11), (7, 11)))


def u_shape():
    return _plane(HAND_SHAPE, ((2, 3), (8, 3)), ((8, 3), (8, 6)), ((2, 6), (8, 6)))


def isolated_beside():
    return _plane(HAND_SHAPE, ((3, 2), (3, 8)), (5, 5))


def unlabelled_between():
    """three collinear runs; the middle one carries label 0"""
    img = _plane(HAND_SHAPE, ((4, 2), (4, 6)), ((4, 9), (4, 13)), ((4, 16), (4, 20)))
    lab = CC.canonical_labels(img)
    lab[4, 9:14] = 0
    return img, lab


def two_planes():
    """an end on the last row of plane 0 and one on the first row of plane 1, in the same column"""
    return _plane((8, 12), ((3, 5), (7, 5))), _plane((8, 12), ((0, 5), (4, 5)))


def borders():
    """short runs along the borders whose ends sit in the four corners, an isolated pixel in the middle of every side"""
    H, W = 16, 21
    return _plane((H, W), ((0, 0), (0, 3)), ((3, 0), (7, 0)), ((H - 1, W - 4), (H - 1, W - 1)), ((H - 8, W - 1), (H - 4, W - 1)), ((0, W - 3), (0, W - 1)),
                  ((H - 1, 0), (H - 1, 2)), (0, 10), (H - 1, 10), (10, 0), (4, W - 1))


def equal_d2(with_first=True):
    """isolated pixels at d2 = 25 around (5, 5) in four rows and on both sides; the raster-first one is (2, 9), without it (5, 0)"""
    pts = [(5, 5), (5, 0), (10, 5), (8, 1), (0, 11)] + [(2, 9)] * with_first
    return _plane((12, 12), *pts)


BRIDGE_PAIRS = (((2, 2), (4, 9)), ((2, 32), (4, 25)), ((14, 2), (21, 4)), ((14, 30), (21, 28)), ((30, 2), (35, 7)), ((30, 32), (35, 27)),
                ((44, 2), (44, 8)), ((44, 25), (50, 25)))


def bridge_pairs():
    """pairs of isolated pixels, each pair further than G = 8 from every other: shallow and steep, to the right and to the left, both
    diagonals, a row and a column"""
    return _plane((56, 36), *[p for pair in BRIDGE_PAIRS for p in pair])


def tile_seams():
    """on SHAPE: ends across the horizontal seam, across the vertical seam, across the four-tile corner, and in the last word's remainder"""
    H, W = SHAPE
    return _plane(SHAPE, ((56, 20), (TH - 2, 20)), ((TH + 2, 20), (H - 1, 20)),                 # (62, 20) / (66, 20)
                  ((10, 118), (10, TW - 2)), ((10, TW + 1), (10, W - 1)),                       # (10, 126) / (10, 129): the run ends in the last column
                  (TH - 2, TW - 2), (TH + 1, TW + 1),                                           # the corner
                  ((30, TW + 1), (34, TW + 1)), ((32, W - 1), (36, W - 1)),                     # both inside the last word
                  ((TH - 1, 60), (TH - 1, 70)), ((TH + 1, 64), (TH + 1, 74)))


def source_grid(n):
    """n isolated pixels in the first tile of SHAPE, 7 rows and 9 columns apart: WAVE_SRC of them take the kernel's wave route, one more
    its lane route"""
    pts = [(3 + 7 * (k // 8), 3 + 9 * (k % 8)) for k in range(n)]
    assert max(y for y, _ in pts) < TH and max(x for _, x in pts) < TW
    return _plane(SHAPE, *pts)


def across_a_tile():
    """on BIG: isolated pixels exactly 64 apart down and across, found at G = 64, and pairs 65 apart, not found"""
    return _plane(BIG, (63, 250), (127, 250), (5, 100), (5, 164), (63, 20), (128, 20), (131, 100), (131, 165))


@functools.lru_cache(maxsize=None)
def crack_case(mask):
    """(topo, labels) [1, H, W] of a broken-crack mask: the topo bytes of its skeleton and the canonical labels of its region"""
    img = CC.broken_cracks(*mask)
    return of_skeleton(SC.skeleton(img), labels=CC.canonical_labels(img))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (topo uint8 [N, H, W], labels int32 [N, H, W]); built once, nothing mutates them"""
    out = {"collinear": of_skeleton(collinear()), "tee": of_skeleton(tee()), "u_shape": of_skeleton(u_shape()),
           "isolated_beside": of_skeleton(isolated_beside()), "two_planes": of_skeleton(*two_planes()), "borders": of_skeleton(borders()),
           "equal_d2": of_skeleton(equal_d2()), "equal_d2_second": of_skeleton(equal_d2(False)), "bridge_pairs": of_skeleton(bridge_pairs()),
           "tile_seams": of_skeleton(tile_seams()), "across_a_tile": of_skeleton(across_a_tile()),
           f"grid_{WAVE_SRC}": of_skeleton(source_grid(WAVE_SRC)), f"grid_{WAVE_SRC + 1}": of_skeleton(source_grid(WAVE_SRC + 1))}
    img, lab = unlabelled_between()
    out["unlabelled_between"] = of_skeleton(img, labels=lab)
    for mask in CRACK_MASKS:
        out["cracks_%d_%dx%d" % mask] = crack_case(mask)
    for d in TC.DENSITIES:
        out[f"noise_{d}"] = of_skeleton(TC.noise(d))
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return out


def gaps_for(name):
    """the G values a case is run with"""
    return NOISE_GAPS if name.startswith("noise") else GAPS


@functools.lru_cache(maxsize=None)
def expected(name, G, to):
    """(gap_q, gap_d2, table, group_labels, bridge_map) of a case"""
    topo, labels = cases()[name]
    gq, gd = gaps_brute(topo, labels, G, to)
    out = (gq, gd, gap_table(topo, labels, gq, gd), groups_of(labels, gq), bridges_of(gq))
    for a in out:
        a.setflags(write=False)
    return out


def gap_dicts(rows, W, crack_of_label=None):
    """the ``gaps`` list of ``predict_dataset`` from one plane's rows, by a loop"""
    out = []
    for _, p, q, d2, la, lb, cq, mutual in np.asarray(rows, np.int64).reshape(-1, 8).tolist():
        d = dict(y=p // W, x=p % W, to=(q // W, q % W), gap_px=float(np.sqrt(np.float64(d2))), d2=d2, kind="end_end" if cq in (1, 2) else "end_side",
                 mutual=bool(mutual))
        if crack_of_label is not None:
            d.update(crack=crack_of_label[la], to_crack=crack_of_label[lb])
        out.append(d)
    return out
