"""Spur pruning (csrc/prune.hip, utils/estimate_metrics.prune_spurs, predict_dataset(prune_spur_px=)) restated in NumPy, and the cases of
tests/test_prune_cpu.py and tests/test_prune_gpu.py.

With the ring N, NE, E, SE, S, SW, W, NW of topology_cases, n8 the set neighbours and A the ring positions where a clear neighbour is
followed by a set one, a set pixel is a TIP iff A == 1 and n8 <= 3, and ISOLATED iff n8 == 0.  Everything outside a plane is clear.

  peel  : X_0 = S; for k = 1 .. L: E = the tips of X_(k-1), D_k = the pixels of E with an 8-neighbour in X_(k-1) \\ E, X_k = X_(k-1) \\ D_k,
          T = k on D_k (0 where nothing was peeled)
  seeds : Z = the tips and isolated pixels of X_L, M(z) = the largest T among z's 8 neighbours
  grow  : R empty; for k = L .. 1: R gains every q with T(q) = k that has an 8-neighbour r with (r in Z and M(r) = k) or (r in R and
          T(r) = k + 1)
  P = X_L | R

``prune`` is the definition by shifted planes, ``prune_brute`` the same pixel by pixel over sets of coordinates, and ``tiled`` the same
computed the way the kernels do: tile by tile, a fixed number of steps per launch, with everything outside a tile's halo taken as clear."""
import functools

import numpy as np

import skeleton_cases as SC
import topology_cases as TC

TH, TW, WORD = 64, 128, 32                                # csrc/prune.hip: PR_TH, 32 * PR_TWW, bits of a word
KP, KG = 8, 16                                            # PR_KP, PR_KG: the steps per launch of the peel and the grow kernel
MAX_SPUR = 64
SHAPE = SC.SHAPE                                          # 70 x 133
SHAPES = ((1, 1), (1, 12), (12, 1), (5, 7), (64, 128), (65, 129), (70, 133), (130, 260))
DENSITIES = (0.05, 0.3, 0.6, 0.95)
CRACK_SEEDS = TC.CRACK_SEEDS
RING = TC.RING
_shift = TC._shift


def spur_lengths(kp=KP, kg=KG):
    """the L of the device tests: around the launch-group boundaries of both kernels (the grow kernel runs the steps L - 1 .. 1, so its
    second launch begins at L = kg + 2), without duplicates, ascending"""
    return tuple(sorted({1, 2, kp - 1, kp, kp + 1, 2 * kp + 1, kg + 1, kg + 2, 33, 64}))


# ------------------------------------------------------------------------------------------------------------ the definition
def _ring(s):
    return [_shift(s, dy, dx) for dy, dx in RING]


def tips_of(plane):
    """(tips, isolated) bool planes"""
    s = np.asarray(plane) != 0
    r = _ring(s)
    n8 = sum(k.astype(np.int64) for k in r)
    A = sum((~r[i] & r[(i + 1) % 8]).astype(np.int64) for i in range(8))
    return s & (A == 1) & (n8 <= 3), s & (n8 == 0)


def _sum8(t):
    """(the sum is exactly 1, the sum is at least 4) of eight bool planes the way the kernel forms them: two full adders and a half adder for
    the ones, then the four carries, which weigh 2 each"""
    full = lambda a, b, c: (a ^ b ^ c, (a & b) | (c & (a ^ b)))
    s0, c0 = full(t[0], t[1], t[2])
    s1, c1 = full(t[3], t[4], t[5])
    s2, c2 = t[6] ^ t[7], t[6] & t[7]
    a1, c3 = full(s0, s1, s2)
    x2, f0 = full(c0, c1, c2)
    ge4 = f0 | (x2 & c3)
    return a1 & ~(x2 ^ c3) & ~ge4, ge4


def tips_adder_form(plane):
    """the tips through the bit-sliced adders of csrc/prune.hip"""
    s = np.asarray(plane) != 0
    r = _ring(s)
    return s & _sum8([~r[i] & r[(i + 1) % 8] for i in range(8)])[0] & ~_sum8(r)[1]


def _any8(s):
    return functools.reduce(np.logical_or, _ring(s))


def peel_step(x):
    """D: the tips of x with a neighbour that is set and no tip"""
    e = tips_of(x)[0]
    return e & _any8(x & ~e)


def peel(plane, L):
    """(X_L bool, T uint8)"""
    x = np.asarray(plane) != 0
    t = np.zeros(x.shape, np.uint8)
    for k in range(1, L + 1):
        d = peel_step(x)
        if not d.any():                                   # a fixed point: the remaining steps delete nothing either
            break
        x = x & ~d
        t[d] = k
    return x, t


def seeds_of(x, t):
    """(Z bool, M uint8): the tips and isolated pixels of x, and the largest T among each pixel's neighbours"""
    e, iso = tips_of(x)
    return e | iso, functools.reduce(np.maximum, _ring(t))


def grow(x, t, L):
    """R bool"""
    z, m = seeds_of(x, t)
    r = np.zeros(x.shape, bool)
    for k in range(L, 0, -1):
        r |= (t == k) & _any8((z & (m == k)) | (r & (t == k + 1)))
    return r


def prune(plane, L):
    """(P uint8 0 / 1, X_L uint8 0 / 1, T uint8) of one plane"""
    x, t = peel(plane, L)
    return (x | grow(x, t, L)).astype(np.uint8), x.astype(np.uint8), t


def prune_of(planes, L):
    """(P [N, H, W], T [N, H, W], removed int32 [N]) of a stack of planes"""
    res = [prune(p, L) for p in planes]
    out, t = np.stack([r[0] for r in res]), np.stack([r[2] for r in res])
    removed = (np.asarray(planes) != 0).sum(axis=(1, 2)) - out.sum(axis=(1, 2))
    return out, t, removed.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ pixel by pixel
def _nbrs(p):
    return [(p[0] + dy, p[1] + dx) for dy, dx in RING]


def _is_tip(p, x):
    ring = [q in x for q in _nbrs(p)]
    return sum(ring) <= 3 and sum(1 for i in range(8) if not ring[i] and ring[(i + 1) % 8]) == 1


def prune_brute(plane, L):
    """the same three planes from sets of coordinates"""
    s = np.asarray(plane) != 0
    x = {(int(y), int(x_)) for y, x_ in np.argwhere(s)}
    t = {}
    for k in range(1, L + 1):
        e = {p for p in x if _is_tip(p, x)}
        d = {p for p in e if any(q in x and q not in e for q in _nbrs(p))}
        x -= d
        t.update({p: k for p in d})
    z = {p for p in x if _is_tip(p, x) or not any(q in x for q in _nbrs(p))}
    m = {p: max(t.get(q, 0) for q in _nbrs(p)) for p in z}
    r = set()
    for k in range(L, 0, -1):
        r |= {q for q, tq in t.items() if tq == k and any((p in z and m[p] == k) or (p in r and t[p] == k + 1) for p in _nbrs(q))}
    out, xl, tt = (np.zeros(s.shape, np.uint8) for _ in range(3))
    for p in x:
        out[p] = xl[p] = 1
    for p in r:
        out[p] = 1
    for p, k in t.items():
        tt[p] = k
    return out, xl, tt


# ------------------------------------------------------------------------------------------------------------ tile by tile
def _window(a, y0, y1, x0, x1):
    """a[y0:y1, x0:x1] with zeros where the window leaves the plane"""
    H, W = a.shape
    out = np.zeros((y1 - y0, x1 - x0), a.dtype)
    ya, yb, xa, xb = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = a[ya:yb, xa:xb]
    return out


def tiled(plane, L, th=TH, tw=TW, kp=KP, kg=KG, halo_x=WORD):
    """(P, X_L, T) the way csrc/prune.hip computes them.  Peel: launches of up to ``kp`` steps; a workgroup owns th x tw pixels, loads them with
    2 kp rows and ``halo_x`` >= 2 kp columns per side, takes everything else as clear, peels locally, and writes only what it owns to the
    other plane.  Seeds: straight from the definition (that kernel has no tile).  Grow: launches of up to ``kg`` of the steps L - 1 .. 1 with
    a halo of kg pixels."""
    assert halo_x >= 2 * kp
    s = np.asarray(plane) != 0
    H, W = s.shape
    origins = [(y, x) for y in range(0, H, th) for x in range(0, W, tw)]
    x, t = s.copy(), np.zeros(s.shape, np.uint8)
    for k0 in range(0, L, kp):
        nxt = np.zeros_like(x)
        for y0, x0 in origins:
            win = _window(x, y0 - 2 * kp, y0 + th + 2 * kp, x0 - halo_x, x0 + tw + halo_x)
            own = (slice(2 * kp, 2 * kp + th), slice(halo_x, halo_x + tw))
            for k in range(k0 + 1, min(k0 + kp, L) + 1):
                d = peel_step(win)
                if not d.any():
                    break
                win = win & ~d
                dst = t[y0:y0 + th, x0:x0 + tw]
                dst[d[own][:dst.shape[0], :dst.shape[1]]] = k
            dst = nxt[y0:y0 + th, x0:x0 + tw]
            dst[...] = win[own][:dst.shape[0], :dst.shape[1]]
        x = nxt
    z, m = seeds_of(x, t)
    r = np.zeros(s.shape, bool)
    for dy, dx in RING:                                                      # q is restored by a seed z next to it with M(z) = T(q)
        r |= (t > 0) & _shift(z, dy, dx) & (_shift(m, dy, dx) == t)
    k_hi = L - 1
    while k_hi >= 1:
        k_lo = max(k_hi - kg + 1, 1)
        nxt = np.zeros_like(r)
        for y0, x0 in origins:
            box = (y0 - kg, y0 + th + kg, x0 - kg, x0 + tw + kg)
            wt, wr = _window(t, *box), _window(r, *box)
            for k in range(k_hi, k_lo - 1, -1):
                wr = wr | ((wt == k) & _any8(wr & (wt == k + 1)))
            dst = nxt[y0:y0 + th, x0:x0 + tw]
            dst[...] = wr[kg:kg + th, kg:kg + tw][:dst.shape[0], :dst.shape[1]]
        r = nxt
        k_hi = k_lo - 1
    return (x | r).astype(np.uint8), x.astype(np.uint8), t


# ------------------------------------------------------------------------------------------------------------ what must hold
def holes(plane):
    return TC.holes(plane)


def properties_hold(plane, L):
    """the five properties of the issue for one plane and one L (the fifth against L - 1); returns the number of removed pixels"""
    s = np.asarray(plane) != 0
    p, xl, _ = prune(s, L)
    p, xl = p != 0, xl != 0
    assert not (xl & ~p).any() and not (p & ~s).any()
    assert SC.components(p) == SC.components(s)
    assert holes(p) == holes(s)
    assert np.array_equal(prune(p, L)[0] != 0, p)
    removed = int(s.sum() - p.sum())
    if L > 1:
        assert removed >= int(s.sum() - prune(s, L - 1)[0].sum())
    return removed


# ------------------------------------------------------------------------------------------------------------ shapes
def _pts(shape, pts):
    img = np.zeros(shape, np.uint8)
    for y, x in pts:
        img[y, x] = 1
    return img


def run_with_spur(y=0, x=0, run=19, spur=3, vertical=False):
    """a T: a run of ``run`` pixels and a spur of ``spur`` pixels that stands on its middle; (y, x) is the run's first pixel.  With
    ``vertical`` the run goes down and the spur to the right"""
    pts = [(0, i) for i in range(run)] + [(1 + j, run // 2) for j in range(spur)]
    return [(y + b, x + a) if vertical else (y + a, x + b) for a, b in pts]


def fork(y, x, run=20, arms=(5, 3)):
    """a run of ``run`` pixels to the right from (y, x) whose last pixel carries two diagonal arms, up of arms[0] and down of arms[1] pixels"""
    end = x + run - 1
    return [(y, x + i) for i in range(run)] + [(y - j, end + j) for j in range(1, arms[0] + 1)] + [(y + j, end + j) for j in range(1, arms[1] + 1)]


def ring_with_tail(y, x, side=8, tail=12):
    """the outline of a side x side square with its corner at (y, x) and a tail of ``tail`` pixels to the right from the middle of its side"""
    pts = [(y + i, x + j) for i in range(side) for j in range(side) if i in (0, side - 1) or j in (0, side - 1)]
    return pts + [(y + side // 2, x + side + j) for j in range(tail)]


HAND_SHAPE = (24, 40)
# name -> (points in a 24 x 40 plane, {L: removed pixels})
HAND = {
    "T_19_3": (run_with_spur(4, 5), {1: 0, 2: 0, 3: 3, 4: 3, 5: 3}),
    "fork_5_3": (fork(10, 3), {1: 0, 2: 0, **{L: 3 for L in range(3, 11)}}),
    "fork_3_3": (fork(10, 3, arms=(3, 3)), {L: 0 for L in (1, 2, 3, 4, 5, 8, 16, 64)}),
    "segments": ([(2, 3)] + [(5, 3), (5, 4)] + [(8, 3), (9, 4), (10, 4)], {16: 0}),
    "ring_tail": (ring_with_tail(6, 4), {**{L: 0 for L in (1, 5, 11)}, **{L: 12 for L in (12, 13, 20, 64)}}),
    "block": ([(3, 4), (3, 5), (4, 4), (4, 5)], {1: 0, 16: 0}),
}
# seed -> {L: removed pixels}, and the tips that are left
FIXTURE_REMOVED = {0: {1: 1, 4: 11, 8: 11, 16: 11, 64: 205}, 1: {1: 0, 4: 4, 8: 17, 16: 93, 64: 153}, 2: {1: 2, 4: 4, 8: 9, 16: 38, 64: 166}}
FIXTURE_TIPS_0 = {0: 9, 1: 8, 4: 5, 8: 5, 16: 5, 64: 0}


def hand(name):
    return _pts(HAND_SHAPE, HAND[name][0])


def noise(density, shape=SHAPE, seed=23):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def crack_skeleton(seed):
    return TC.crack_skeleton(seed)


def placed(pts, shape=SHAPE):
    return _pts(shape, [p for p in pts if 0 <= p[0] < shape[0] and 0 <= p[1] < shape[1]])


def corners():
    """uint8 [4, 70, 133]: the hand shapes pushed against the plane's corners and borders -- a run along the first row with its spur
    hanging down, one along the last column, a fork that ends in the last column, a ring in the bottom right corner"""
    H, W = SHAPE
    a = placed(run_with_spur(0, 0) + run_with_spur(H - 4, W - 19))
    b = placed(run_with_spur(0, W - 4, vertical=True) + run_with_spur(H - 19, 0, vertical=True))
    c = placed(fork(5, W - 25) + fork(H - 4, 0, arms=(5, 3)))
    d = placed(ring_with_tail(H - 8, W - 20) + ring_with_tail(0, 0))
    return np.stack([a, b, c, d])


def seam_spurs(L):
    """uint8 [3, 90 + 2 L, 160 + 3 L]: spurs of L - 1, L and L + 1 pixels (plane 0, 1, 2; at least one pixel) that cross a tile seam, base in
    one tile and tip in the next -- a vertical run left of the column seam 127 | 128 with a spur to the right, and a horizontal run above the
    row seam 63 | 64 with a spur downwards.  The runs reach L + 10 pixels beyond the spur on both sides, so their own ends never meet it:
    pruning with L removes both spurs of plane 0 and 1 and leaves plane 2 as it is"""
    out = []
    for n in (max(L - 1, 1), L, L + 1):
        pts = [(y, 126) for y in range(2, 2 * L + 23)] + [(L + 12, 127 + j) for j in range(n)]
        pts += [(62, x) for x in range(135 + L, 135 + 3 * L + 21)] + [(63 + j, 145 + 2 * L) for j in range(n)]
        out.append(_pts((90 + 2 * L, 160 + 3 * L), pts))
    return np.stack(out)


def long_spur():
    """uint8 [1, 130, 260]: two spurs of 40 pixels -- longer than the halo of one peel launch (16) and of one grow launch (16) --, one down from
    a run of 200 over the row seam at 64, one to the left from a run of 105 over the column seam 127 | 128"""
    pts = [(10, x) for x in range(20, 220)] + [(11 + j, 100) for j in range(40)]
    pts += [(y, 150) for y in range(20, 125)] + [(72, 149 - j) for j in range(40)]
    return _pts((130, 260), pts)[None]


def seam_shapes():
    """uint8 [3, 70, 133]: a fork whose junction lies on the corner of four tiles and one on the word seam 31 | 32; 2 x 2 blocks across the
    row seam, the column seam and the corner; 2-pixel segments that straddle each seam"""
    a = placed(fork(64, 128 - 19, arms=(4, 2)) + fork(20, 32 - 19, arms=(5, 3)) + fork(40, 64 - 19, arms=(3, 3)))
    b = placed([(y, x) for y0, x0 in ((63, 10), (20, 127), (63, 127), (30, 31)) for y in (y0, y0 + 1) for x in (x0, x0 + 1)])
    c = placed([(63, 20), (64, 20), (10, 127), (10, 128), (63, 127), (64, 128), (40, 31), (40, 32), (63, 60), (64, 61)])
    return np.stack([a, b, c])


def thin_between_full():
    """uint8 [3, 20, 45]: a thin plane between two full ones"""
    x = np.ones((3, 20, 45), np.uint8)
    x[1] = _pts((20, 45), run_with_spur(2, 3) + fork(14, 2, run=20, arms=(5, 3))) * 200
    return x


@functools.lru_cache(maxsize=None)
def cases():
    """name -> uint8 [N, H, W], for every L"""
    out = {f"hand_{k}": hand(k)[None] for k in HAND}
    out["corners"] = corners()
    out["long_spur"] = long_spur()
    out["seam_shapes"] = seam_shapes()
    for d in DENSITIES:
        out[f"noise_{d}"] = noise(d)[None]
    for h, w in SHAPES:
        out[f"noise_{h}x{w}"] = np.stack([noise(0.3, (h, w), 3), noise(0.6, (h, w), 4)])
    out["ones_1x1"] = np.ones((1, 1, 1), np.uint8)
    out["ones"] = np.ones((1,) + SHAPE, np.uint8)
    out["zeros"] = np.zeros((1,) + SHAPE, np.uint8)
    out["cracks"] = np.stack([crack_skeleton(s) for s in CRACK_SEEDS])
    out["thin_between_full"] = thin_between_full()
    out["w33"] = np.stack([noise(0.3, (9, 33), 5), _pts((9, 33), run_with_spur(2, 14))])
    out["w31"] = np.stack([noise(0.3, (9, 31), 6), _pts((9, 31), run_with_spur(2, 12))])
    return out


@functools.lru_cache(maxsize=None)
def expected(name, L):
    """(P, T, removed) of a case, computed once"""
    planes = seam_spurs(L) if name == "seam_spurs" else cases()[name]
    return prune_of(planes, L)
