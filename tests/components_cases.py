"""Connected components, the per-component table and the small-component filter (csrc/components.hip, utils/estimate_metrics.label_components
/ component_table / keep_components, predict_dataset(min_crack_px=)) restated in NumPy / SciPy, and the cases of tests/test_components_cpu.py
and tests/test_components_gpu.py.

``canonical_labels`` is the definition: scipy.ndimage.label, relabelled to 1 + the smallest linear index of the component.  ``tiled_labels``
is the form the kernel takes -- a union-find per TH x TW tile with the kernel's choice of pairs (one lane per WORD pixels of a row), one merge
over the seam pixels with the kernel's choice of pairs, a flatten -- and the CPU test holds it equal to the definition on every case.

The kernel's workgroup owns TH x TW pixels: the seams lie at y = 64 and x = 128, and the shapes below leave a few pixels behind each."""
import functools

import numpy as np

import skeleton_cases as SC

TH, TW, WORD = 64, 128, 32                                # csrc/components.hip: CC_TH, 32 * CC_TWW, bits of a word
SHAPE = (TH + 6, TW + 5)                                  # 70 x 133
DENSITIES = (0.2, 0.3, 0.45, 0.6)
NOISE_SEED = 7
COLUMNS = ("plane", "label", "area_px", "skeleton_px", "y0", "x0", "y1", "x1")


# ------------------------------------------------------------------------------------------------------------ the definition
def canonical_labels(img, connectivity=8):
    """int32 [H, W] of a bool plane: 0 for background, 1 + min(y W + x) over its component for a set pixel"""
    from scipy.ndimage import label
    img = np.asarray(img).astype(bool)
    assert img.ndim == 2 and connectivity in (4, 8)
    lab, n = label(img, structure=np.ones((3, 3), int) if connectivity == 8 else None)
    first = np.full(n + 1, img.size, np.int64)
    np.minimum.at(first, lab.ravel(), np.arange(img.size))
    return np.where(lab > 0, first[lab] + 1, 0).astype(np.int32)


def labels_of(planes, threshold, connectivity=8):
    """int32 [N, H, W]: the canonical labels of every binarised plane"""
    return np.stack([canonical_labels(SC.binarise(p, threshold), connectivity) for p in planes])


def table(labels, skeleton=None, min_px=1):
    """int32 [M, 8] = (plane, label, area_px, skeleton_px, y0, x0, y1, x1) per component with area_px >= min_px, sorted by (plane, label);
    the box is inclusive, skeleton_px counts the non-zero ``skeleton`` pixels inside the component (0 without one)"""
    labels = np.asarray(labels)
    N, H, W = labels.shape
    rows = []
    yy, xx = np.mgrid[:H, :W]
    for n in range(N):
        flat = labels[n].ravel().astype(np.int64)
        area = np.bincount(flat, minlength=H * W + 1)
        sk = np.zeros(H * W + 1, np.int64) if skeleton is None else np.bincount(flat, weights=(np.asarray(skeleton[n]).ravel() != 0),
                                                                                minlength=H * W + 1).astype(np.int64)
        lo_y, lo_x = np.full(H * W + 1, H), np.full(H * W + 1, W)
        hi_y, hi_x = np.full(H * W + 1, -1), np.full(H * W + 1, -1)
        np.minimum.at(lo_y, flat, yy.ravel())
        np.minimum.at(lo_x, flat, xx.ravel())
        np.maximum.at(hi_y, flat, yy.ravel())
        np.maximum.at(hi_x, flat, xx.ravel())
        for lab in np.nonzero(area[1:])[0] + 1:
            if area[lab] >= min_px:
                rows.append((n, lab, area[lab], sk[lab], lo_y[lab], lo_x[lab], hi_y[lab], hi_x[lab]))
    return np.array(rows, np.int32).reshape(-1, 8)


def keep(labels, min_px):
    """uint8 [N, H, W]: 1 where the pixel's component has >= min_px pixels"""
    labels = np.asarray(labels)
    out = np.zeros(labels.shape, np.uint8)
    for n in range(labels.shape[0]):
        area = np.bincount(labels[n].ravel(), minlength=labels[n].size + 1)
        out[n] = (labels[n] > 0) & (area[labels[n]] >= min_px)
    return out


def cracks_of(table_rows, W):
    """the ``cracks`` list of predict_dataset from the rows of one plane, in plain Python"""
    out = []
    for _, lab, area, length, y0, x0, y1, x1 in np.asarray(table_rows).tolist():
        out.append(dict(y=(lab - 1) // W, x=(lab - 1) % W, area_px=area, length_px=length, mean_width_px=area / length if length else 0.0,
                        bbox=(y0, x0, y1, x1)))
    return out


# ------------------------------------------------------------------------------------------------------------ the kernel's form
def _find(L, i):
    while L[i] < i:
        i = L[i]
    return i


def _union(L, a, b):
    """the kernel's union by smaller index, sequentially: the larger root's slot is lowered to the smaller root"""
    a, b = _find(L, a), _find(L, b)
    if a != b:
        L[max(a, b)] = min(a, b)


def _shift(a, dy, dx):
    """a[y + dy, x + dx], False outside"""
    H, W = a.shape
    p = np.pad(a, 1)
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def tile_local(img, connectivity, word=WORD):
    """parents of one tile, local raster indices (-1: background), after the local pass: runs inside a word hang on their first pixel, then
    the unions the kernel makes -- a run continuing from the word to the left, one north union per pair of touching runs, the two diagonals
    only under a background pixel and only where the horizontal neighbour does not make the join"""
    h, w = img.shape
    L = np.full(h * w, -1, np.int64)
    for y in range(h):
        start = 0
        for x in range(w):
            if img[y, x]:
                if x % word == 0 or not img[y, x - 1]:
                    start = y * w + x
                L[y * w + x] = start
    c, u = img, _shift(img, -1, 0)
    cw, ce, uw, ue = _shift(img, 0, -1), _shift(img, 0, 1), _shift(img, -1, -1), _shift(img, -1, 1)
    word_start = (np.arange(w) % word == 0)[None, :]
    for y, x in np.argwhere(c & cw & word_start):
        _union(L, y * w + x, y * w + x - 1)
    for y, x in np.argwhere(c & u & ~(cw & uw)):
        _union(L, y * w + x, (y - 1) * w + x)
    if connectivity == 8:
        for y, x in np.argwhere(c & ~u & uw & ~cw):
            _union(L, y * w + x, (y - 1) * w + x - 1)
        for y, x in np.argwhere(c & ~u & ue & ~ce):
            _union(L, y * w + x, (y - 1) * w + x + 1)
    return L.reshape(h, w)


def tiled_labels(img, connectivity=8, th=TH, tw=TW):
    """local labelling per th x tw tile (the global index of the tile-local root per set pixel, -1 for background), one merge over the seam
    pixels with the kernel's pairs, flatten: int32 [H, W]"""
    img = np.asarray(img).astype(bool)
    H, W = img.shape
    L = np.full(H * W, -1, np.int64)
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            t = img[y0:y0 + th, x0:x0 + tw]
            loc = tile_local(t, connectivity)
            for y, x in np.argwhere(t):
                root = _find(loc.ravel(), y * t.shape[1] + x)
                L[(y0 + y) * W + x0 + x] = (y0 + root // t.shape[1]) * W + x0 + root % t.shape[1]
    on = lambda y, x: 0 <= y < H and 0 <= x < W and img[y, x]
    for y in range(th, H, th):                            # horizontal seams, one lane per pixel of the row below
        for x in range(W):
            if not img[y, x]:
                continue
            p = y * W + x
            if on(y - 1, x):
                if not (on(y, x - 1) and on(y - 1, x - 1)):
                    _union(L, p, p - W)
            elif connectivity == 8:
                if on(y - 1, x - 1):
                    _union(L, p, p - W - 1)
                if on(y - 1, x + 1):
                    _union(L, p, p - W + 1)
    for x in range(tw, W, tw):                            # vertical seams, one lane per pixel of the column to the right
        for y in range(H):
            if not img[y, x]:
                continue
            p = y * W + x
            if on(y, x - 1):
                _union(L, p, p - 1)
            elif connectivity == 8:
                if on(y - 1, x - 1):
                    _union(L, p, p - 1 - W)
                if on(y + 1, x - 1):
                    _union(L, p, p - 1 + W)
    out = np.zeros(H * W, np.int32)
    for i in np.nonzero(L >= 0)[0]:
        out[i] = _find(L, i) + 1
    return out.reshape(H, W)


# ------------------------------------------------------------------------------------------------------------ inputs
def _pixels(shape, pts):
    img = np.zeros(shape, bool)
    for y, x in pts:
        img[y, x] = True
    return img


def u_shape(orientation):
    """two arms that cross a seam and meet only on its far side: 'down' / 'up' cross y = TH with the bar below / above it, 'right' / 'left'
    cross x = TW with the bar right / left of it"""
    img = np.zeros(SHAPE, bool)
    if orientation in ("down", "up"):
        img[TH - 4:TH + 4, 20] = img[TH - 4:TH + 4, 29] = True
        img[TH + 3 if orientation == "down" else TH - 4, 20:30] = True
    else:
        img[20, TW - 4:TW + 4] = img[29, TW - 4:TW + 4] = True
        img[20:30, TW + 3 if orientation == "right" else TW - 4] = True
    return img


def comb(vertical_seam):
    """20 teeth in one tile, one pixel apart, joined only by a spine in the next tile: 19 unions onto one root"""
    img = np.zeros(SHAPE, bool)
    if vertical_seam:
        img[4:44:2, TW - 9:TW] = True                     # horizontal teeth left of x = TW
        img[4:43, TW] = True
    else:
        img[TH - 9:TH, 4:44:2] = True                     # vertical teeth above y = TH
        img[TH, 4:43] = True
    return img


def serpentine():
    """every second row full, joined alternately at the two ends: one path through the whole plane"""
    H, W = SHAPE
    img = np.zeros(SHAPE, bool)
    img[0::2] = True
    for k, y in enumerate(range(1, H, 2)):
        img[y, W - 1 if k % 2 == 0 else 0] = True
    return img


def spiral():
    """a one-pixel rectangular spiral with one-pixel gaps, from the border inwards"""
    H, W = SHAPE
    img = np.zeros(SHAPE, bool)
    blocked = lambda y, x: not (0 <= y < H and 0 <= x < W)
    ahead = lambda y, x, d, k: (y + k * d[0], x + k * d[1])
    dirs, k, (y, x) = [(0, 1), (1, 0), (0, -1), (-1, 0)], 0, (0, 0)
    img[0, 0] = True
    while True:
        for turn in (0, 1):                                # walk on; at a wall or one pixel before the previous turn of the spiral, turn right
            d = dirs[(k + turn) % 4]
            n1, n2 = ahead(y, x, d, 1), ahead(y, x, d, 2)
            if not blocked(*n1) and not img[n1] and (blocked(*n2) or not img[n2]):
                break
        else:
            return img
        k, (y, x) = (k + turn) % 4, n1
        img[y, x] = True


def checkerboard():
    yy, xx = np.mgrid[:SHAPE[0], :SHAPE[1]]
    return (yy + xx) % 2 == 0


def noise(density, seed=NOISE_SEED):
    return np.random.default_rng(seed).random(SHAPE) < density


def broken_cracks(seed, H, W):
    """random-walk cracks through every seam, cut by three zeroed columns and three zeroed rows"""
    img = SC.random_walk_cracks(seed, H, W).copy()
    for f in (0.2, 0.5, 0.8):
        img[:, int(W * f)] = False
        img[int(H * f), :] = False
    return img


def crosses_seams(labels, th=TH, tw=TW):
    """(components with pixels on both sides of y = th, ... of x = tw) of one label plane"""
    a = set(np.unique(labels[:th])) & set(np.unique(labels[th:])) - {0}
    b = set(np.unique(labels[:, :tw])) & set(np.unique(labels[:, tw:])) - {0}
    return len(a), len(b)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (fp32 planes [N, H, W], threshold); built once, nothing mutates them."""
    H, W = SHAPE
    f = SC._f32
    c = {}
    c["1x1_set"] = f(np.ones((1, 1, 1), bool))
    c["1x1_clear"] = f(np.zeros((1, 1, 1), bool))
    c["1xW_line"] = f(np.ones((1, 1, W), bool))
    c["Hx1_line"] = f(np.ones((1, H, 1), bool))
    c["zeros"] = f(np.zeros((1, H, W), bool))
    c["ones"] = f(np.ones((1, H, W), bool))
    c["width_33"] = f(np.random.default_rng(33).random((1, 9, 33)) < 0.6)              # one word and one pixel
    c["width_19"] = f(SC.random_walk_cracks(3, H, 19)[None])                          # narrower than a word
    c["corner_diagonal"] = f(_pixels(SHAPE, [(TH - 1, TW - 1), (TH, TW)])[None])       # contact only across the corner of four tiles
    c["corner_anti_diagonal"] = f(_pixels(SHAPE, [(TH - 1, TW), (TH, TW - 1)])[None])
    c["hseam_diagonals"] = f(_pixels(SHAPE, [(TH - 1, 10), (TH, 11), (TH - 1, 21), (TH, 20)])[None])
    c["vseam_diagonals"] = f(_pixels(SHAPE, [(10, TW - 1), (11, TW), (21, TW - 1), (20, TW)])[None])
    for o in ("down", "up", "right", "left"):
        c[f"u_{o}"] = f(u_shape(o)[None])
    c["comb_hseam"] = f(comb(False)[None])
    c["comb_vseam"] = f(comb(True)[None])
    c["serpentine"] = f(serpentine()[None])
    c["spiral"] = f(spiral()[None])
    c["checkerboard"] = f(checkerboard()[None])
    for d in DENSITIES:
        c[f"noise_{d}"] = f(noise(d)[None])
    c["cracks_2_vseams"] = f(broken_cracks(2, TH + 3, 2 * TW + 7)[None])
    c["cracks_2_hseams"] = f(broken_cracks(6, 2 * TH + 3, TW + 7)[None])
    cracks = broken_cracks(4, H, W)
    c["batch5"] = f(np.stack([SC.corner_blob(H, W), cracks, np.zeros((H, W), bool), np.random.default_rng(5).random((H, W)) < 0.5, cracks]))
    out = {k: (v, 0.5) for k, v in c.items()}
    pred, _, t = SC.pair()
    out["pair_special_values"] = (pred, t)                 # NaN, +-inf, the threshold and its neighbours
    return out


@functools.lru_cache(maxsize=None)
def expected(name, connectivity=8):
    """int32 [N, H, W]: the canonical labels of a case, computed once per process and shared by the tests"""
    planes, t = cases()[name]
    return labels_of(planes, t, connectivity)


@functools.lru_cache(maxsize=None)
def expected_skeleton(name):
    planes, t = cases()[name]
    return SC.skeleton_of(planes, t)
