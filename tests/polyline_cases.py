"""The crack polylines (csrc/polylines.hip, utils/estimate_metrics.order_branches / branch_polylines / arc_position / polyline_stats,
predict_dataset(polylines=)) restated in NumPy, and the cases of tests/test_polylines_cpu.py and tests/test_polylines_gpu.py.

All terms are those of tests/branch_cases.py.  The DEGREE of a branch pixel is the number of its inner links; a branch is a CHAIN when no
pixel of it has a degree above 2.  A chain with terminals (degree <= 1) is a path and starts at the terminal with the smaller linear index;
a chain without one is a cycle, starts at its first pixel (blabel - 1) and is walked from there first to the start's neighbour with the
smaller linear index.  rank = the inner links walked from the start, diag = the SE / SW links among them, both -1 at clear pixels, at
junction pixels and at every pixel of a branch that is no chain.

``walk`` is the definition, one step per pixel; ``jump_form`` the same the way the kernel forms it: two half-states per pixel of a compact
list, doubled in rounds that read one buffer and write the other."""
import functools
import math

import numpy as np

import branch_cases as BC
import topology_cases as TC

SQRT2 = float(np.sqrt(2.0))
STOP = 2
ORDER_COLUMNS = ("y", "x", "diag", "d2")


# ------------------------------------------------------------------------------------------------------------ the definition
def neighbours(topo):
    """{p: [(q, diagonal), ...]} over the inner links of one plane's topo, both ways, and the branch pixels in raster order"""
    nb = {int(p): [] for p in np.nonzero(BC.is_branch(topo).ravel())[0]}
    for p, q, k in BC.partition(topo)[0]:
        nb[p].append((q, int(k >= 2)))
        nb[q].append((p, int(k >= 2)))
    return nb


def chains_of(nb, blabels):
    """{label: (pixels, is a chain, the terminals)} of one plane"""
    flat = np.asarray(blabels).ravel()
    out = {}
    for p in nb:
        out.setdefault(int(flat[p]), []).append(p)
    return {lab: (px, all(len(nb[p]) <= 2 for p in px), [p for p in px if len(nb[p]) <= 1]) for lab, px in out.items()}


def walk(topo, blabels):
    """(rank, diag) int32 [H, W] of one plane by a walk along every chain from its start"""
    t = np.asarray(topo)
    nb = neighbours(t)
    rank, diag = (np.full(t.size, -1, np.int32) for _ in range(2))
    for lab, (px, chain, terminals) in chains_of(nb, blabels).items():
        if not chain:
            continue
        assert len(terminals) in (0, 2) or len(px) == 1, "a path has two terminals or is one pixel"
        start = min(terminals) if terminals else lab - 1
        assert start in px
        rank[start] = diag[start] = 0
        if len(px) == 1:
            continue
        at, (nxt, dg) = start, min(nb[start])                                        # a terminal's only neighbour; a cycle's smaller one
        r = d = 0
        while nxt != start and rank[nxt] < 0:
            r, d = r + 1, d + dg
            rank[nxt], diag[nxt] = r, d
            step = [(q, g) for q, g in nb[nxt] if q != at]
            if not step:
                break
            at, (nxt, dg) = nxt, step[0]
        assert r == len(px) - 1, "the walk visits every pixel of the chain"
    return rank.reshape(t.shape), diag.reshape(t.shape)


def jump_form(topo, blabels, rounds=None):
    """(rank, diag, rounds) the way the kernel forms it.  The branch pixels are a compact list; every pixel keeps two half-states, one per
    side: (the slot reached, links walked, diagonal links walked, the side through which to go on or STOP, the side entered).  A round reads
    buffer A and writes buffer B -- every half-state that has not stopped appends the half-state of the slot it has reached -- and the buffers
    swap.  ``rounds`` None: as many rounds as change something (returned); else exactly that many, as the device does with ceil(log2(P))."""
    t = np.asarray(topo)
    flat = np.asarray(blabels).ravel()
    nb = neighbours(t)
    pix = np.array(sorted(nb), np.int64)
    P = pix.size
    rank, diag = (np.full(t.size, -1, np.int32) for _ in range(2))
    if P == 0:
        return rank.reshape(t.shape), diag.reshape(t.shape), 0
    slot = {int(p): k for k, p in enumerate(pix)}
    ns = np.full((P, 2), -1, np.int64)
    dg = np.zeros((P, 2), np.int64)
    deg = np.array([len(nb[int(p)]) for p in pix])
    for k, p in enumerate(pix):
        for s, (q, g) in enumerate(nb[int(p)][:2]):
            ns[k, s], dg[k, s] = slot[q], g
    root = np.array([slot[int(flat[p]) - 1] for p in pix])
    flags = np.zeros(P, np.int64)
    np.bitwise_or.at(flags, root, (deg > 2) * 1 | (deg <= 1) * 2)
    chain, terminals = (flags[root] & 1) == 0, (flags[root] & 2) != 0
    stop = (deg <= 1) | (~terminals & (root == np.arange(P)))
    # a half-state: at, links, diagonal links, go on through (or STOP), entered through
    A = np.zeros((P, 2, 5), np.int64)
    A[:, :, 0] = np.arange(P)[:, None]
    A[:, :, 3] = STOP
    for s in range(2):
        q = ns[:, s]
        ok = chain & (q >= 0)
        en = np.where(ns[q, 0] == np.arange(P), 0, 1)
        assert (ns[q[ok], en[ok]] == np.arange(P)[ok]).all(), "the links are symmetric"
        A[ok, s] = np.stack([q, np.ones(P, np.int64), dg[:, s], np.where(stop[q], STOP, 1 - en), en], 1)[ok]
    done = 0
    while rounds is None or done < rounds:
        go = A[:, :, 3] != STOP
        if rounds is None and not go.any():
            break
        B = A.copy()                                                                 # the other buffer: a round reads only A
        nxt = A[A[:, :, 0], np.where(go, A[:, :, 3], 0)]
        B[go] = np.stack([nxt[..., 0], A[..., 1] + nxt[..., 1], A[..., 2] + nxt[..., 2], nxt[..., 3], nxt[..., 4]], -1)[go]
        A, done = B, done + 1
    assert (A[:, :, 3] == STOP).all(), "every half-state has reached its stop"
    for k in np.nonzero(chain)[0]:
        a, b = A[k]
        if terminals[k]:
            pick = a if pix[a[0]] <= pix[b[0]] else b
        elif k == root[k]:
            pick = (k, 0, 0)
        else:
            side = 0 if pix[ns[root[k], 0]] < pix[ns[root[k], 1]] else 1              # the walk leaves the root through its smaller neighbour
            pick = a if a[4] == side else b
            assert pick[0] == root[k]
        rank[pix[k]], diag[pix[k]] = pick[1], pick[2]
    return rank.reshape(t.shape), diag.reshape(t.shape), done


def rounds_bound(n):
    """ceil(log2(n)) + 1 for n pixels"""
    return (math.ceil(math.log2(n)) if n > 1 else 0) + 1


def longest_chain(topo, blabels):
    return max([len(px) for px, chain, _ in chains_of(neighbours(np.asarray(topo)), blabels).values() if chain], default=0)


# ------------------------------------------------------------------------------------------------------------ the tables
def polylines_of(blabels, rank, diag, d2=None):
    """(chain bool [M], offsets int64 [M + 1], points int32 [P_chain, 4]) of planes [N, H, W]: the rows of the branch table, sorted by
    (plane, label); a chain's span holds (y, x, diag, d2 or 0) of its pixels in the order of rank, a non-chain's is empty"""
    blabels, rank, diag = (np.asarray(a) for a in (blabels, rank, diag))
    N, H, W = blabels.shape
    chain, offsets, points = [], [0], []
    for n in range(N):
        flat, rk = blabels[n].ravel(), rank[n].ravel()
        for lab in np.unique(flat[flat != 0]):
            idx = np.nonzero(flat == lab)[0]
            ok = bool(rk[lab - 1] >= 0)
            assert ((rk[idx] >= 0) == ok).all(), "a branch is ordered as a whole or not at all"
            chain.append(ok)
            if ok:
                idx = idx[np.argsort(rk[idx])]
                assert np.array_equal(rk[idx], np.arange(idx.size))
                dd = np.zeros(idx.size, np.int64) if d2 is None else np.asarray(d2)[n].ravel()[idx]
                points.append(np.stack([idx // W, idx % W, diag[n].ravel()[idx], dd], 1))
            offsets.append(offsets[-1] + (idx.size if ok else 0))
    pts = np.concatenate(points).astype(np.int32) if points else np.zeros((0, 4), np.int32)
    return np.array(chain, bool), np.array(offsets, np.int64), pts.reshape(-1, 4)


def cycles_of(topo, blabels):
    """the labels of one plane's chains without a terminal"""
    return {lab for lab, (px, chain, terminals) in chains_of(neighbours(np.asarray(topo)), blabels).items() if chain and not terminals}


def arc_of(rank, diag):
    return float((rank - diag) + SQRT2 * diag)


def stats_of(points, cycle=False):
    """the figures of polyline_stats of one branch's points [px, >= 2] (y, x first), in plain Python"""
    pts = [(int(p[0]), int(p[1])) for p in np.asarray(points).reshape(-1, np.shape(points)[-1] if np.ndim(points) == 2 else 2)]
    if not pts:
        return dict(start=None, stop=None, arc_px=0.0, chord_px=0.0, tortuosity=None, direction_deg=None)
    nd = sum(1 for a, b in zip(pts, pts[1:]) if a[0] != b[0] and a[1] != b[1])
    arc = arc_of(len(pts) - 1, nd)
    dy, dx = pts[-1][0] - pts[0][0], pts[-1][1] - pts[0][1]
    chord = float(math.sqrt(float(dy * dy + dx * dx)))
    return dict(start=pts[0], stop=pts[-1], arc_px=arc, chord_px=chord, tortuosity=None if chord == 0 or cycle else arc / chord,
                direction_deg=None if chord == 0 else math.degrees(math.atan2(dy, dx)) % 180.0)


def polyline_dicts(topo, blabels, rank, diag, d2=None):
    """the keys predict_dataset(polylines=True) adds to every dict of ``branches``, for one plane, in the order of the branch table"""
    topo, blabels = np.asarray(topo), np.asarray(blabels)
    chain, offsets, points = polylines_of(blabels[None], np.asarray(rank)[None], np.asarray(diag)[None], None if d2 is None else np.asarray(d2)[None])
    labels = np.unique(blabels[blabels != 0])
    cycles = cycles_of(topo, blabels)
    out = []
    for j, lab in enumerate(labels):
        pts = points[offsets[j]:offsets[j + 1]]
        d = dict(chain=bool(chain[j]), points=pts[:, :2].copy(), **stats_of(pts, int(lab) in cycles))
        if d2 is not None:
            d["width_profile_px"] = np.array([BC.width_of_d2(v) for v in pts[:, 3]], np.float64)
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------------------ shapes
def serpentine(H, W):
    """uint8 [H, W]: the rows 0, 2, 4, ... joined alternately at the last and at the first column -- one path through every tile seam"""
    a = np.zeros((H, W), np.uint8)
    a[0::2] = 1
    for k, y in enumerate(range(1, H - 1, 2)):
        a[y, W - 1 if k % 2 == 0 else 0] = 1
    return a


def staircase():
    """uint8 [9, 11]: steps of one E and one SE link, so that diag differs from rank"""
    a = np.zeros(TC.HAND_SHAPE, np.uint8)
    y, x = 1, 1
    a[y, x] = 1
    for k in range(8):
        x += 1
        if k % 2:
            y += 1
        a[y, x] = 1
    return a


def pixel_between_junctions():
    """uint8 [9, 11]: two pluses whose facing arms leave one branch pixel between the two junction pixels"""
    return TC._pts(TC.HAND_SHAPE, TC.at(TC.plus(1), 4, 4) + TC.at(TC.plus(1), 4, 6))


def corner_rings():
    """uint8 [2, 70, 133]: a square ring and a diamond centred on the corner (64, 128) of four tiles"""
    sq = [(y, x) for y in range(-3, 4) for x in range(-3, 4) if abs(y) == 3 or abs(x) == 3]
    di = [(y, x) for y in range(-4, 5) for x in range(-4, 5) if abs(y) + abs(x) == 4]
    return np.stack([TC._pts(TC.SHAPE, TC.at(sq, 64, 128)), TC._pts(TC.SHAPE, TC.at(di, 64, 128))])


def swapped_planes():
    """two batches uint8 [2, 70, 133] with the same two planes in either order: a plane that read its neighbour would show"""
    a, b = TC.crack_skeleton(0), corner_rings()[1]
    return np.stack([a, b]), np.stack([b, a])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> uint8 [N, H, W] planes: all of branch_cases.cases() and the shapes above"""
    out = dict(BC.cases())
    out["serpentine_130x260"] = serpentine(130, 260)[None]
    out["serpentine_66x130"] = serpentine(66, 130)[None]
    out["staircase"] = staircase()[None]
    out["hand_diag7"] = TC.hand("diag7")[None]
    out["pixel_between_junctions"] = pixel_between_junctions()[None]
    out["corner_rings"] = corner_rings()
    out["swapped_ab"], out["swapped_ba"] = swapped_planes()
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(topo uint8, blabels int32, rank int32, diag int32, rounds) of a case, each [N, H, W], computed once by the jump form; rounds is the
    largest of the planes"""
    topo = np.stack([TC.topo_of(p) for p in cases()[name]])
    bl = np.stack([BC.blabels_of(t) for t in topo])
    res = [jump_form(t, b) for t, b in zip(topo, bl)]
    return topo, bl, np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), max(r[2] for r in res)
