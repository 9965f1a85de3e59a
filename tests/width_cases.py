"""The local crack width (csrc/width.hip, utils/estimate_metrics.skeleton_width / component_width_table / summarize_width_hist,
predict_dataset(width_radius=)) restated in NumPy / SciPy, and the cases of tests/test_width_cpu.py and tests/test_width_gpu.py.

``d2_of`` is the definition: scipy.ndimage.distance_transform_edt's index of the nearest background pixel, the squared distance taken as
integers from the indices, clipped to r^2 + 1; a plane without background is r^2 + 1 everywhere.  Nothing outside the plane is background.
``kernel_form`` is the form the kernel takes -- per TH x TW tile the bit-packed region with a halo of r rows and ceil(r / 32) words per
side, positions outside the plane set, and a row-by-row walk that finds the nearest clear bit a word at a time -- and the CPU test holds
it equal to the definition.

The kernel's workgroup owns TH x TW pixels: the seams lie at y = 64 and x = 128, and the shapes below leave a few pixels behind each."""
import functools

import numpy as np

import components_cases as CC
import skeleton_cases as SC

TH, TW, WORD = 64, 128, 32                                # csrc/width.hip: WD_TH, 32 * WD_TWW, bits of a word
MAX_RADIUS = 128
SHAPE = (TH + 6, TW + 5)                                  # 70 x 133
BIG = (3 * TH + 6, 2 * TW + 5)                            # 198 x 261: the disks
RADII = (1, 5, 33, 64, 128)
BAR_WIDTHS = tuple(range(1, 10))


# ------------------------------------------------------------------------------------------------------------ the definition
def d2_of(region, r):
    """int32 [H, W]: min(r^2 + 1, squared distance to the nearest pixel of the plane outside ``region``), 0 at a pixel outside it"""
    from scipy.ndimage import distance_transform_edt
    region = np.asarray(region).astype(bool)
    cap = r * r + 1
    if region.all():
        return np.full(region.shape, cap, np.int32)
    iy, ix = distance_transform_edt(region, return_distances=False, return_indices=True)
    yy, xx = np.mgrid[:region.shape[0], :region.shape[1]]
    d = (iy.astype(np.int64) - yy) ** 2 + (ix.astype(np.int64) - xx) ** 2
    return np.minimum(d, cap).astype(np.int32)


def d2_brute(region, r):
    """the same by a double loop over the pixels"""
    region = np.asarray(region).astype(bool)
    H, W = region.shape
    bg = np.argwhere(~region)
    out = np.zeros((H, W), np.int32)
    for y in range(H):
        for x in range(W):
            best = r * r + 1
            for by, bx in bg:
                best = min(best, (by - y) ** 2 + (bx - x) ** 2)
            out[y, x] = best
    return out


def width_of(planes, skeleton, threshold, r):
    """(d2 int32 [N, H, W] masked by the skeleton, hist int32 [N, r^2 + 2] over the skeleton pixels)"""
    planes, skeleton = np.asarray(planes), np.asarray(skeleton)
    d2 = np.stack([np.where(s != 0, d2_of(SC.binarise(p, threshold), r), 0) for p, s in zip(planes, skeleton)]).astype(np.int32)
    hist = np.stack([np.bincount(d[s != 0], minlength=r * r + 2) for d, s in zip(d2, skeleton)]).astype(np.int32)
    return d2, hist


def width_rows(labels, d2, min_px=1):
    """int32 [M, 5] = (plane, label, max_d2, y, x) per component of at least min_px pixels, sorted by (plane, label): the largest d2 over the
    component, the first pixel in raster order that attains it; (0, -1, -1) for a component without a pixel of d2 > 0"""
    labels, d2 = np.asarray(labels), np.asarray(d2)
    N, H, W = labels.shape
    rows = []
    for n in range(N):
        flat, d = labels[n].ravel().astype(np.int64), d2[n].ravel().astype(np.int64)
        area = np.bincount(flat, minlength=H * W + 1)
        best = np.zeros(H * W + 1, np.int64)
        np.maximum.at(best, flat, d)
        first = np.full(H * W + 1, H * W, np.int64)
        hit = (d > 0) & (d == best[flat])
        np.minimum.at(first, flat[hit], np.nonzero(hit)[0])
        for lab in np.nonzero(area[1:])[0] + 1:
            if area[lab] >= min_px:
                y, x = divmod(int(first[lab]), W) if best[lab] > 0 else (-1, -1)
                rows.append((n, lab, best[lab], y, x))
    return np.array(rows, np.int32).reshape(-1, 5)


def width(d2):
    """the local width, plain Python: 2 sqrt(d2) - 1, 0.0 for d2 = 0"""
    return 2.0 * float(np.sqrt(np.float64(d2))) - 1.0 if d2 > 0 else 0.0


def summary(d2_values, r):
    """the figures of summarize_width_hist from the list of the skeleton pixels' d2, by sorting"""
    v = np.sort(np.asarray(d2_values, np.int64))
    out = {"outside_px": int((v == 0).sum()), "saturated_px": int((v == r * r + 1).sum())}
    v = v[v > 0]
    n = len(v)
    out["centerline_px"] = n
    if n == 0:
        out.update(centerline_width_px=0.0, median_width_px=0.0, p95_width_px=0.0, max_width_px=0.0)
        return out
    w = [width(int(d)) for d in v]
    out.update(centerline_width_px=sum(w) / n, median_width_px=w[(n - 1) // 2], p95_width_px=w[-(-95 * n // 100) - 1], max_width_px=w[-1])
    return out


# ------------------------------------------------------------------------------------------------------------ the kernel's form
def _clz(v):
    return 32 - int(v).bit_length()


def _ctz(v):
    return (int(v) & -int(v)).bit_length() - 1


def kernel_form(region, skeleton, r, th=TH, tw=TW):
    """d2 int32 [H, W] the way the kernel computes it: per tile, words of 32 pixels with a halo, outside the plane set"""
    region, skeleton = np.asarray(region).astype(bool), np.asarray(skeleton) != 0
    H, W = region.shape
    hw = (r + 31) // 32
    wpr = tw // 32 + 2 * hw
    cap = r * r + 1
    out = np.zeros((H, W), np.int32)
    M = 0xFFFFFFFF
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            pts = np.argwhere(skeleton[y0:y0 + th, x0:x0 + tw])
            if len(pts) == 0:
                continue
            rows = th + 2 * r
            gy = np.arange(y0 - r, y0 - r + rows)[:, None]
            gx = np.arange(x0 - 32 * hw, x0 - 32 * hw + 32 * wpr)[None, :]
            inside = (gy >= 0) & (gy < H) & (gx >= 0) & (gx < W)
            px = np.where(inside, region[np.clip(gy, 0, H - 1), np.clip(gx, 0, W - 1)], True)
            bits = (px.reshape(rows, wpr, 32) * (1 << np.arange(32, dtype=np.int64))).sum(-1)
            for ly, lx in pts:
                row, bx = ly + r, lx + 32 * hw
                cw, b = bx >> 5, bx & 31
                best, dy = cap, 0
                while dy * dy < best:
                    for rr in ((row,) if dy == 0 else (row - dy, row + dy)):
                        R = bits[rr]
                        inv = ~int(R[cw]) & M
                        left = inv & (M >> (31 - b))
                        if left:
                            best = min(best, dy * dy + (b - 31 + _clz(left)) ** 2)
                        else:
                            for j in range(1, hw + 1):
                                if dy * dy + (32 * (j - 1) + b + 1) ** 2 >= best:
                                    break
                                w = ~int(R[cw - j]) & M
                                if w:
                                    best = min(best, dy * dy + (32 * j + b - 31 + _clz(w)) ** 2)
                                    break
                        right = inv & ((M << b) & M)
                        if right:
                            best = min(best, dy * dy + (_ctz(right) - b) ** 2)
                        else:
                            for j in range(1, hw + 1):
                                if dy * dy + (32 * j - b) ** 2 >= best:
                                    break
                                w = ~int(R[cw + j]) & M
                                if w:
                                    best = min(best, dy * dy + (32 * j + _ctz(w) - b) ** 2)
                                    break
                    dy += 1
                out[y0 + ly, x0 + lx] = best
    return out


# ------------------------------------------------------------------------------------------------------------ inputs
def bar(kind, w, shape=SHAPE):
    """a straight bar of width w from border to border through the tile seams: 'h' across y = TH, 'v' across x = TW, 'd' / 'a' the two
    diagonals through the corner (TH, TW) (w pixels measured along x)"""
    H, W = shape
    img = np.zeros(shape, bool)
    yy, xx = np.mgrid[:H, :W]
    if kind == "h":
        img[TH - w // 2:TH - w // 2 + w, :] = True
    elif kind == "v":
        img[:, TW - w // 2:TW - w // 2 + w] = True
    else:
        c = (xx - TW) - (yy - TH) if kind == "d" else (xx - TW) + (yy - TH)
        img[(c >= -(w // 2)) & (c < w - w // 2)] = True
    return img


def disk(cy, cx, radius, shape=BIG):
    yy, xx = np.mgrid[:shape[0], :shape[1]]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius


def exact_distance(r, shape):
    """(region [2, H, W], skeleton [2, H, W]): all set but one background pixel, one skeleton pixel; the background at (0, r) from it -- d2 =
    r^2, not saturated -- and at (r, 1) -- d2 = r^2 + 1, saturated"""
    H, W = shape
    y, x = 2, min(TW - r // 2 - 1, W - r - 2)             # the pair straddles x = TW, and y = TH from r = 64 on
    assert y + r < H and x + r < W
    reg, sk = np.ones((2, H, W), bool), np.zeros((2, H, W), np.uint8)
    reg[0, y, x + r] = False
    reg[1, y + r, x + 1] = False
    sk[:, y, x] = 1
    return reg, sk


def cross():
    """a 5-wide row and a 3-wide column from border to border: the crack touches all four borders"""
    img = np.zeros(SHAPE, bool)
    img[30:35, :] = True
    img[:, 90:93] = True
    return img


def _sk(region):
    return SC.skeleton(region).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (fp32 planes [N, H, W], uint8 skeleton [N, H, W], threshold, the radii the case runs at); built once, nothing mutates them."""
    H, W = SHAPE
    f = SC._f32
    c = {}

    def add(name, regions, skeleton=None, radii=RADII):
        regions = np.asarray(regions)
        sk = np.stack([_sk(g) for g in regions]) if skeleton is None else np.asarray(skeleton, np.uint8)
        c[name] = (f(regions), sk, 0.5, tuple(radii))

    for kind in "hvda":
        add(f"bars_{kind}", np.stack([bar(kind, w) for w in BAR_WIDTHS]))
    add("cracks", SC.random_walk_cracks(1, H, W)[None])
    add("cracks_2_vseams", SC.random_walk_cracks(2, TH + 3, 2 * TW + 7)[None])
    for d in (0.3, 0.6):
        add(f"noise_{d}", CC.noise(d)[None])
    add("disk40_corner", disk(2 * TH, TW, 40)[None], radii=(33, 64, 128))           # the halo spans more than one tile and more than one word
    add("disk70", disk(100, 130, 70)[None], radii=(64,))                            # the centre is saturated
    for r in (1, 5, 33, 64):
        add(f"exact_r{r}", *exact_distance(r, SHAPE), radii=(r,))
    add("exact_r128", *exact_distance(128, (2 * TH + 12, 2 * TW + 5)), radii=(128,))
    add("four_borders", cross()[None])
    last = np.zeros(SHAPE, bool)
    last[:, W - 3:] = True                                                          # W % 32 = 5: the crack in the last columns of the last word
    edge = np.zeros((1, H, W), np.uint8)
    edge[0, :, W - 1] = 1                                                           # measured in the last column: 3 from the background, 1 from the padding
    add("last_columns", last[None], skeleton=edge)
    add("ones", np.ones((1, H, W), bool))
    add("zeros", np.zeros((1, H, W), bool))
    add("1x1_set", np.ones((1, 1, 1), bool))
    add("1x1_clear", np.zeros((1, 1, 1), bool), skeleton=np.ones((1, 1, 1), np.uint8))                # a skeleton pixel outside R
    add("5x7", np.random.default_rng(57).random((1, 5, 7)) < 0.6, radii=(128, 1))
    rng = np.random.default_rng(12)
    add("skeleton_outside", CC.noise(0.45)[None], skeleton=(rng.random((1, H, W)) < 0.1))              # about half of it in bin 0
    cracks = SC.random_walk_cracks(4, H, W)
    add("batch5", np.stack([SC.corner_blob(H, W), cracks, np.zeros((H, W), bool), np.random.default_rng(5).random((H, W)) < 0.5,
                            np.ones((H, W), bool)]))
    pred, _, t = SC.pair()                                 # NaN, +-inf, the threshold and its neighbours
    c["pair_special_values"] = (pred, SC.skeleton_of(pred, t), t, RADII)
    return c


def case_radii():
    """(name, r) for every case and every radius it runs at, sorted"""
    return [(name, r) for name in sorted(cases()) for r in cases()[name][3]]


@functools.lru_cache(maxsize=None)
def expected(name, r):
    """(d2, hist) of a case at radius r, computed once per process and shared by the tests"""
    planes, sk, t, _ = cases()[name]
    return width_of(planes, sk, t, r)


@functools.lru_cache(maxsize=None)
def expected_labels(name):
    planes, _, t, _ = cases()[name]
    return CC.labels_of(planes, t, 8)


@functools.lru_cache(maxsize=None)
def many_tiles():
    """(region bool [1000, 1100], skeleton uint8): random-walk cracks dilated to mixed widths -- squares of 1 .. 15 pixels stamped along them"""
    from scipy.ndimage import binary_dilation
    H, W = 1000, 1100
    rng = np.random.default_rng(64)
    img = np.zeros((H, W), bool)
    for k, w in enumerate((1, 3, 6, 9, 15)):
        thin = np.zeros((H, W), bool)
        y, x = float(rng.integers(0, H)), 0
        while x < W:
            thin[int(min(max(y, 0), H - 1)), x] = True
            x += 1
            y += rng.integers(-1, 2)
        x, y = float(rng.integers(0, W)), 0
        while y < H:
            thin[y, int(min(max(x, 0), W - 1))] = True
            y += 1
            x += rng.integers(-1, 2)
        img |= binary_dilation(thin, structure=np.ones((w, w), bool)) if w > 1 else thin
    return img, _sk(img)
