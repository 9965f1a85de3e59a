"""Guo-Hall parallel thinning, the centerline counts and the clDice scores (csrc/skeleton.hip, utils/estimate_metrics.skeletonize /
centerline_counts, inference.cldice_scores) restated in NumPy, and the cases of tests/test_skeleton_cpu.py and tests/test_skeleton_gpu.py.

``sub_iteration`` is the definition, written with the eight shifted neighbour planes and the formulas of DESIGN 1.10 as they stand;
``skeleton`` iterates it over the whole plane; ``tiled`` is the form the kernel takes -- K passes on independent tiles that carry a halo
of 2 K pixels, only the tile interior kept -- and the CPU test holds its fixed point equal to ``skeleton``.

The kernel's workgroup owns TH x TW pixels and runs at most K passes per launch, on rows packed WORD pixels to a word: the seams lie at
y = 64 and x = 128, and the shapes below leave a remainder of a few pixels behind each seam."""
import csv
import functools

import numpy as np

TH, TW, K, WORD = 64, 128, 8, 32                          # csrc/skeleton.hip: SK_TH, 32 * SK_TWW, SK_K, bits of a word
SEAM_Y, SEAM_X = TH, TW
SHAPE = (TH + 6, TW + 5)                                  # 70 x 133: one seam in each direction and a remainder that is no multiple of a word


# ------------------------------------------------------------------------------------------------------------ the definition
def sub_iteration(img, second):
    """one sub-iteration on a bool plane [H, W]: (the new plane, the number of deleted pixels).  Pixels outside the image are 0."""
    H, W = img.shape
    p = np.pad(img.astype(bool), 1)
    at = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    P2, P3, P4, P5, P6, P7, P8, P9 = at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1)
    i = lambda a: a.astype(np.int64)
    C = i(~P2 & (P3 | P4)) + i(~P4 & (P5 | P6)) + i(~P6 & (P7 | P8)) + i(~P8 & (P9 | P2))
    N1 = i(P9 | P2) + i(P3 | P4) + i(P5 | P6) + i(P7 | P8)
    N2 = i(P2 | P3) + i(P4 | P5) + i(P6 | P7) + i(P8 | P9)
    N = np.minimum(N1, N2)
    m = ((P6 | P7 | ~P9) & P8) if second else ((P2 | P3 | ~P5) & P4)
    delete = img.astype(bool) & (C == 1) & (N >= 2) & (N <= 3) & ~m
    return img.astype(bool) & ~delete, int(delete.sum())


def one_pass(img):
    a, d0 = sub_iteration(img, 0)
    b, d1 = sub_iteration(a, 1)
    return b, d0 + d1


def skeleton(img, max_passes=0, return_passes=False):
    """the plane after the first pass that deletes nothing, or after min(max_passes, that many) passes when max_passes > 0.
    ``return_passes``: also the number of passes run, the one that deleted nothing included."""
    cur, n = np.asarray(img).astype(bool), 0
    while max_passes == 0 or n < max_passes:
        cur, deleted = one_pass(cur)
        n += 1
        if deleted == 0:
            break
    return (cur, n) if return_passes else cur


def tiled(img, k, th, tw):
    """k passes on every th x tw tile separately, each with a halo of 2 k pixels (zero outside the image), the tile interiors kept:
    (the new plane, the number of deleted pixels)"""
    img = np.asarray(img).astype(bool)
    H, W = img.shape
    h = 2 * k
    p = np.pad(img, h)
    out = np.zeros_like(img)
    for y0 in range(0, H, th):
        for x0 in range(0, W, tw):
            t = p[y0:min(y0 + th, H) + 2 * h, x0:min(x0 + tw, W) + 2 * h]
            for _ in range(k):
                t, _ = one_pass(t)
            out[y0:y0 + th, x0:x0 + tw] = t[h:-h, h:-h]
    return out, int(img.sum() - out.sum())


def tiled_skeleton(img, k, th, tw):
    """``tiled`` groups until one deletes nothing: (the plane, the number of groups, that one included)"""
    cur, groups = np.asarray(img).astype(bool), 0
    while True:
        cur, deleted = tiled(cur, k, th, tw)
        groups += 1
        if deleted == 0:
            return cur, groups


def components(img):
    """number of 8-connected components"""
    from scipy.ndimage import label
    return int(label(np.asarray(img).astype(bool), structure=np.ones((3, 3), int))[1])


# ------------------------------------------------------------------------------------------------------------ counts and scores
def binarise(x, threshold):
    """x - threshold > 0 in fp32, NaN -> False"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, np.float32) - np.float32(threshold)) > 0


def skeleton_of(planes, threshold, max_passes=0):
    """uint8 [N, H, W]: the skeleton of every binarised plane"""
    return np.stack([skeleton(binarise(p, threshold), max_passes) for p in planes]).astype(np.uint8)


def counts(pred, mask, threshold):
    """int64 [N, 4] = (|S_P|, |S_P & V_L|, |S_L|, |S_L & V_P|) with V_P = pred - t > 0, V_L = mask > 0.5 and S their skeletons"""
    out = np.zeros((pred.shape[0], 4), np.int64)
    for n in range(pred.shape[0]):
        vp, vl = binarise(pred[n], threshold), np.asarray(mask[n], np.float32) > np.float32(0.5)
        sp, sl = skeleton(vp), skeleton(vl)
        out[n] = sp.sum(), (sp & vl).sum(), sl.sum(), (sl & vp).sum()
    return out


def scores_naive(c):
    """(Tprec, Tsens, clDice) as lists of Python floats, row by row"""
    out = ([], [], [])
    for n_sp, sp_in, n_sl, sl_in in np.asarray(c).tolist():
        tp = sp_in / n_sp if n_sp else 1.0
        ts = sl_in / n_sl if n_sl else 1.0
        cl = 2.0 * tp * ts / (tp + ts) if tp + ts > 0 else 0.0
        for lst, v in zip(out, (tp, ts, cl)):
            lst.append(v)
    return out


def read_csv(path):
    with open(path, newline="") as fh:
        return list(csv.reader(fh))


# ------------------------------------------------------------------------------------------------------------ inputs
def random_walk_cracks(seed, H, W):
    """bool [H, W]: random-walk cracks 1 .. 5 pixels wide, from border to border, through every tile seam and the seam crossing"""
    rng = np.random.default_rng(seed)
    img = np.zeros((H, W), bool)

    def stamp(y, x, w):
        y0, x0 = int(y) - (w - 1) // 2, int(x) - (w - 1) // 2
        img[max(0, y0):max(0, y0 + w), max(0, x0):max(0, x0 + w)] = True

    for w in (1, 2, 3, 4, 5):
        y, x = float(rng.integers(0, H)), 0.0               # left border to right border: crosses every vertical seam
        while x < W:
            stamp(min(max(y, 0), H - 1), x, w)
            x += 1
            y = min(max(y + rng.integers(-1, 2), 0), H - 1)
        y, x = 0.0, float(rng.integers(0, W))               # top border to bottom border: crosses every horizontal seam
        while y < H:
            stamp(y, min(max(x, 0), W - 1), w)
            y += 1
            x = min(max(x + rng.integers(-1, 2), 0), W - 1)
    for i in range(-8, 9):                                  # a 3-wide diagonal through the corner where four tiles meet
        if SEAM_Y + i < H and SEAM_X + i < W:
            stamp(SEAM_Y + i, SEAM_X + i, 3)
    return img


def corner_blob(H, W):
    """a disk of radius 2 * (2 K) + 3 centred on the corner where four tiles meet: wider than twice the halo, several launch groups"""
    yy, xx = np.mgrid[:H, :W]
    r = 4 * K + 3
    return (yy - SEAM_Y) ** 2 + (xx - SEAM_X) ** 2 <= r * r


def _f32(img, lo=0.0, hi=1.0):
    """a bool plane as an fp32 map: ``hi`` where set, ``lo`` elsewhere"""
    return np.where(img, np.float32(hi), np.float32(lo)).astype(np.float32)


def _at(shape, y, x, block):
    img = np.zeros(shape, bool)
    b = np.asarray(block, bool)
    img[y:y + b.shape[0], x:x + b.shape[1]] = b
    return img


def diagonal_stroke(anti):
    """12 x 12: a 2-pixel-wide diagonal stroke of length 8 (15 pixels) -- the pixels (i, i) and (i, i + 1); ``anti``: upside down"""
    img = np.zeros((12, 12), bool)
    for i in range(8):
        img[2 + i, 2 + i] = True
        if i < 7:
            img[2 + i, 3 + i] = True
    return img[::-1].copy() if anti else img


@functools.lru_cache(maxsize=None)
def cases():
    """name -> fp32 planes [N, H, W] to be binarised at 0.5; built once, nothing mutates them."""
    H, W = SHAPE
    c = {}
    c["1x1_set"] = _f32(np.ones((1, 1, 1), bool))
    c["1x1_clear"] = _f32(np.zeros((1, 1, 1), bool))
    c["1xW_line"] = _f32(np.ones((1, 1, W), bool))
    c["Hx1_line"] = _f32(np.ones((1, H, 1), bool))
    c["3x3_full"] = _f32(np.ones((1, 3, 3), bool))
    c["3x3_cross"] = _f32(np.array([[[0, 1, 0], [1, 1, 1], [0, 1, 0]]], bool))
    c["zeros"] = _f32(np.zeros((1, H, W), bool))
    c["ones_33x129"] = _f32(np.ones((1, 33, 129), bool))
    c["block_2x2"] = _f32(_at((6, 6), 2, 2, np.ones((2, 2)))[None])
    c["rect_5x9"] = _f32(_at((11, 15), 3, 3, np.ones((5, 9)))[None])
    c["diagonal"] = _f32(diagonal_stroke(False)[None])
    c["anti_diagonal"] = _f32(diagonal_stroke(True)[None])
    c["bar_3x8_three_borders"] = _f32(_at((3, 12), 0, 0, np.ones((3, 8)))[None])
    c["cracks"] = _f32(random_walk_cracks(1, H, W)[None])
    c["cracks_2_seams"] = _f32(random_walk_cracks(2, TH + 3, 2 * TW + 7)[None])        # two vertical seams, 263 = 8 words + 7 pixels
    c["corner_blob"] = _f32(corner_blob(2 * TH - 3, 2 * TW - 7)[None])
    c["noise_37x70"] = _f32((np.random.default_rng(37).random((1, 37, 70)) < 0.5))
    c["narrow_70x19"] = _f32(random_walk_cracks(3, H, 19)[None])                       # narrower than a word
    c["width_33"] = _f32(np.random.default_rng(33).random((1, 9, 33)) < 0.6)            # one word and one pixel
    # a batch whose planes converge after different numbers of passes: a blob, thin cracks, nothing, noise
    c["batch4"] = _f32(np.stack([corner_blob(H, W), random_walk_cracks(4, H, W), np.zeros((H, W), bool),
                                 np.random.default_rng(5).random((H, W)) < 0.5]))
    return c


@functools.lru_cache(maxsize=None)
def expected(name, max_passes=0):
    """uint8 [N, H, W]: the skeletons of a case, computed once per process and shared by the tests"""
    return skeleton_of(cases()[name], 0.5, max_passes)


@functools.lru_cache(maxsize=None)
def pair():
    """(pred [3, 70, 133] fp32, mask fp32, threshold 0.3): model-like maps against crack masks -- the cracks widened and shifted, with soft
    values around the threshold, NaN, +-inf; image 2 has an empty mask, and its prediction a blob"""
    H, W = SHAPE
    rng = np.random.default_rng(11)
    masks, preds = [], []
    for n in range(3):
        gt = random_walk_cracks(20 + n, H, W) if n < 2 else np.zeros((H, W), bool)
        m = _f32(gt)
        soft = rng.random((H, W))
        if n < 2:
            m[(soft < 0.02) & ~gt] = 0.5                              # not ground truth
            m[(soft > 0.98) & ~gt] = 0.51                             # ground truth
        base = np.roll(gt, (1 + n, -1), axis=(0, 1)) if n < 2 else corner_blob(H, W)
        p = (rng.random((H, W)) * 0.29).astype(np.float32)
        p[base] = (0.31 + 0.6 * rng.random(int(base.sum()))).astype(np.float32)
        if n == 1:
            p[:, SEAM_X - 2:SEAM_X + 2] = 0.1                         # the predicted crack is broken at the seam
        flat = p.reshape(-1)
        idx = rng.choice(H * W, size=12, replace=False)
        flat[idx] = np.array([np.nan, np.nan, np.inf, -np.inf, 0.3, np.nextafter(np.float32(0.3), np.float32(1)),
                              np.nextafter(np.float32(0.3), np.float32(0)), 0.0, -1.0, 1.5, np.nan, 0.3], np.float32)
        masks.append(m)
        preds.append(p)
    return np.stack(preds), np.stack(masks), 0.3
