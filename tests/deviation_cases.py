"""A CPU oracle for the deviation report (mlsgpu_hip_mesh_deviation), and what its tests share.

deviation() follows the contract in include/mlsgpu_hip.h step by step, with explicit element-wise float64 operations in the
contract's order (no np.dot, einsum, np.cross or linalg: their summation order is not the contract's).  Brute force over all
(point, triangle) pairs runs at about 1.5 M pairs/s, so above PRUNE_ABOVE pairs the candidates of step 2 come from a numpy
grid of the oracle's own: step 2 is then applied exactly to what the grid hands over, as the contract allows any conservative
cull to do.  Nothing here is product code.
"""
import math

import numpy as np

STAT_NAMES = ("numPoints", "numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "within", "beyond",
              "farthestPoint", "farthestChunk", "histogram", "sumQ", "scaleExponent", "maxDistance2", "limit2")
NO_TRIANGLE = 0xFFFFFFFF
NO_POINT = 2 ** 64 - 1
PRUNE_ABOVE = 10 ** 6           # pairs: below this, brute force
BLOCK_PAIRS = 1 << 21           # pairs evaluated at a time
GRID_PAIRS = 1 << 22            # (cell, triangle) pairs the oracle's grid may hold


class Invalid(Exception):
    """What the device reports as MLSGPU_ERR_INVALID."""


# ---------------------------------------------------------------- step 3, on arrays of pairs [N, 3] float64

def _sub(u, v):
    return u[0] - v[0], u[1] - v[1], u[2] - v[2]


def _dot(u, v):
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]


def _cross(u, v):
    return u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]


def _seg(p, a, b):
    u, w = _sub(b, a), _sub(p, a)
    L = _dot(u, u)
    s = np.where(L == 0.0, 0.0, _dot(w, u) / L)
    s = np.fmin(np.fmax(s, 0.0), 1.0)
    r = w[0] - s * u[0], w[1] - s * u[1], w[2] - s * u[2]
    return _dot(r, r)


def _face(p, a, b, c):
    ab, pa = _sub(b, a), _sub(p, a)
    n = _cross(ab, _sub(c, a))
    nn = _dot(n, n)
    i0 = _dot(_cross(ab, pa), n)
    i1 = _dot(_cross(_sub(c, b), _sub(p, b)), n)
    i2 = _dot(_cross(_sub(a, c), _sub(p, c)), n)
    h = _dot(pa, n)
    return np.where((nn > 0.0) & (i0 >= 0.0) & (i1 >= 0.0) & (i2 >= 0.0), (h * h) / nn, np.inf)


def d2(p, a, b, c):
    """Step 3 for N pairs: p, a, b, c are float64 [N, 3] (the floats converted exactly).  float64 [N]."""
    p, a, b, c = (tuple(np.asarray(x, np.float64).reshape(-1, 3).T) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        return np.fmin(np.fmin(np.fmin(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a)), _face(p, a, b, c))


# ---------------------------------------------------------------- steps 1 and 2

def participating(num_vertices, triangles):
    """Step 1: (the indices of the triangles that take part, outOfRangeTriangles, degenerateTriangles)."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    bad = ((tri >= int(num_vertices)) | (tri < 0)).any(axis=1)
    degenerate = ~bad & ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0]))
    return np.flatnonzero(~bad & ~degenerate), int(bad.sum()), int(degenerate.sum())


def _reach(corners, D):
    """lo - D and hi + D per axis of triangles given as float32 [n, 3 corners, 3 axes]: two float64 [n, 3]."""
    lo, hi = corners.min(axis=1).astype(np.float64), corners.max(axis=1).astype(np.float64)
    return lo - D, hi + D


def _candidates(pp, ti, lo, hi, pi):
    """Step 2 for the pairs (pi[k], ti[k]): a mask."""
    x = pp[pi]
    return ((lo[ti] <= x) & (x <= hi[ti])).all(axis=1)


def _brute_pairs(P, n):
    """All pairs, in blocks of at most BLOCK_PAIRS: (point indices, triangle positions)."""
    rows = max(1, BLOCK_PAIRS // max(n, 1))
    for first in range(0, P, rows):
        last = min(P, first + rows)
        pi = np.repeat(np.arange(first, last, dtype=np.int64), n)
        yield pi, np.tile(np.arange(n, dtype=np.int64), last - first)


def _grid_pairs(pp, lo, hi, D):
    """A superset of the candidates from a uniform grid: a triangle goes into every cell from cell(lo - D) to cell(hi + D),
    cell() monotone, so a candidate's point lies in one of them.  Blocks of (point indices, triangle positions)."""
    origin = lo.min(axis=0)
    top = hi.max(axis=0)
    g = max(2.0 * D, float(np.mean((hi - lo).max(axis=1) - 2.0 * D)))
    while True:
        n = np.maximum(np.floor((top - origin) / g).astype(np.int64) + 1, 1)

        def cell(x):
            return np.clip(np.floor((x - origin) / g), 0, n - 1).astype(np.int64)
        c0, c1 = cell(lo), cell(hi)
        span = c1 - c0 + 1
        count = span.prod(axis=1)
        if (n < 2 ** 20).all() and int(count.sum()) <= GRID_PAIRS:
            break
        g *= 2.0
    start = np.cumsum(count) - count
    owner = np.repeat(np.arange(len(count), dtype=np.int64), count)
    k = np.arange(int(count.sum()), dtype=np.int64) - start[owner]
    x = c0[owner, 0] + k % span[owner, 0]
    y = c0[owner, 1] + (k // span[owner, 0]) % span[owner, 1]
    z = c0[owner, 2] + k // (span[owner, 0] * span[owner, 1])
    key = (z * n[1] + y) * n[0] + x
    order = np.argsort(key, kind="stable")
    key, owner = key[order], owner[order]
    pc = cell(pp)
    pkey = (pc[:, 2] * n[1] + pc[:, 1]) * n[0] + pc[:, 0]
    first, last = np.searchsorted(key, pkey, "left"), np.searchsorted(key, pkey, "right")
    length = last - first
    ends = np.cumsum(length)
    at = 0
    while at < len(pp):
        upto = max(at + 1, int(np.searchsorted(ends, (ends[at - 1] if at else 0) + BLOCK_PAIRS, "right")))
        rows = np.arange(at, upto, dtype=np.int64)
        pi = np.repeat(rows, length[rows])
        offset = np.arange(len(pi), dtype=np.int64) - np.repeat(np.cumsum(length[rows]) - length[rows], length[rows])
        yield pi, owner[first[pi] + offset]
        at = upto


def deviation(points, vertices, triangles, D, prune=None):
    """(squared distances float64 [P], nearest triangles uint32 [P], statistics dict) or Invalid.  prune: True / False forces
    the grid or brute force; None chooses by the number of pairs."""
    pf = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    vf = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    D32 = np.float32(D)
    if not (np.isfinite(D32) and D32 > 0):
        raise Invalid("max distance")
    if not np.isfinite(pf).all():
        raise Invalid("point")
    if not np.isfinite(vf).all():
        raise Invalid("vertex")
    D = float(D32)
    D2 = D * D
    P, V, T = len(pf), len(vf), len(tri)
    live, bad, degenerate = participating(V, tri)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats.update(numPoints=P, numVertices=V, numTriangles=T, outOfRangeTriangles=bad, degenerateTriangles=degenerate,
                 farthestPoint=NO_POINT, histogram=[0] * 16, maxDistance2=0.0, limit2=D2)
    best = np.full(P, np.inf)
    nearest = np.full(P, NO_TRIANGLE, np.int64)
    if P == 0:
        return best, nearest.astype(np.uint32), stats
    e = math.frexp(D2)[1] - 1                                   # 2^e <= D2 < 2^(e + 1)
    stats["scaleExponent"] = e

    if len(live):
        corners = vf[tri[live]]                                 # [n, 3 corners, 3 axes]
        lo, hi = _reach(corners, D)
        pp = pf.astype(np.float64)
        ca, cb, cc = (corners[:, k].astype(np.float64) for k in range(3))
        if prune is None:
            prune = P * len(live) > PRUNE_ABOVE
        for pi, ti in (_grid_pairs(pp, lo, hi, D) if prune else _brute_pairs(P, len(live))):
            keep = _candidates(pp, ti, lo, hi, pi)
            pi, ti = pi[keep], ti[keep]
            if len(pi) == 0:
                continue
            d = d2(pp[pi], ca[ti], cb[ti], cc[ti])
            t = live[ti]
            # step 4: per point the smallest distance, then the lowest triangle index that attains it -- against what the
            # earlier blocks left, too.  A candidate counts even at +infinity.
            order = np.lexsort((t, d, pi))
            pi, t, d = pi[order], t[order], d[order]
            head = np.flatnonzero(np.concatenate([[True], pi[1:] != pi[:-1]]))
            pi, t, d = pi[head], t[head], d[head]
            better = (nearest[pi] == NO_TRIANGLE) | (d < best[pi]) | ((d == best[pi]) & (t < nearest[pi]))
            best[pi[better]], nearest[pi[better]] = d[better], t[better]

    within = (nearest != NO_TRIANGLE) & (best <= D2)
    best[~within] = np.inf
    nearest[~within] = NO_TRIANGLE
    w = best[within]
    bins = np.zeros(len(w), np.int64)
    for k in range(1, 16):
        bins = np.where(w >= (D2 * float(k * k)) / 256.0, k, bins)
    stats["within"], stats["beyond"] = int(within.sum()), int((~within).sum())
    stats["histogram"] = [int(x) for x in np.bincount(bins, minlength=16)]
    stats["sumQ"] = int(np.rint(w * 2.0 ** (30 - e)).astype(np.int64).sum())
    if len(w):
        stats["maxDistance2"] = float(w.max())
        stats["farthestPoint"] = int(np.flatnonzero(within & (best == w.max()))[0])
    return best, nearest.astype(np.uint32), stats


def combined(reports):
    """The reports of a sink's dense chunks, in chunk order, as mlsgpu_hip_mesher_deviation adds them up."""
    total = dict.fromkeys(STAT_NAMES, 0)
    total.update(farthestPoint=NO_POINT, histogram=[0] * 16, maxDistance2=0.0)
    for c, one in enumerate(reports):
        for name in ("numPoints", "numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "beyond", "sumQ"):
            total[name] += one[name]
        total["histogram"] = [a + b for a, b in zip(total["histogram"], one["histogram"])]
        total["limit2"] = one["limit2"]
        if one["numPoints"] > 0:
            total["scaleExponent"] = one["scaleExponent"]
        if one["within"] > 0 and (total["within"] == 0 or one["maxDistance2"] > total["maxDistance2"]):
            total.update(maxDistance2=one["maxDistance2"], farthestChunk=c, farthestPoint=one["farthestPoint"])
        total["within"] += one["within"]
    return total


def mean_square(stats):
    """What the host derives from a report: sumQ * 2^(e - 30) / within."""
    return math.ldexp(stats["sumQ"], stats["scaleExponent"] - 30) / stats["within"] if stats["within"] else 0.0


def same_stats(got, want):
    """The report's fields (a dict from the binding may hold derived ones besides), the doubles as bit patterns."""
    g, w = dict((k, got[k]) for k in STAT_NAMES), dict((k, want[k]) for k in STAT_NAMES)
    for k in ("maxDistance2", "limit2"):
        g[k], w[k] = np.float64(g[k]).view(np.uint64), np.float64(w[k]).view(np.uint64)
    assert g == w, (g, w)


def assert_same(got, want):
    """(distances, nearest, stats) against the oracle's: the distances as uint64 bit patterns, the rest exactly.  A None
    among got's arrays (an output the caller did not take) is not compared."""
    gd, gn, gs = got
    wd, wn, ws = want
    same_stats(gs, ws)
    if gd is not None:
        np.testing.assert_array_equal(np.ascontiguousarray(gd, np.float64).view(np.uint64), np.ascontiguousarray(wd, np.float64).view(np.uint64))
    if gn is not None:
        np.testing.assert_array_equal(np.asarray(gn, np.uint32), np.asarray(wn, np.uint32))


# ---------------------------------------------------------------- hand cases: (name, points, vertices, triangles, D)

RIGHT = np.array([[0, 0, 0], [4, 0, 0], [0, 3, 0]], np.float32)


def hand_cases():
    one = np.array([[0, 1, 2]])
    out = [
        ("interior", [[1, 1, 2]], RIGHT, one, 4.0),                     # over the face: 4
        ("edge", [[2, -3, 4]], RIGHT, one, 8.0),                        # beyond side ab: 9 + 16
        ("corner", [[6, -1, 2]], RIGHT, one, 8.0),                      # beyond corner b: 4 + 1 + 4
        ("on_plane", [[1, 1, 0]], RIGHT, one, 1.0),                     # 0
        ("collinear", [[1, 2, 0]], [[0, 0, 0], [2, 0, 0], [4, 0, 0]], one, 4.0),        # zero area: the segments answer, 4
        ("coincident", [[1, 2, 0]], [[0, 0, 0], [0, 0, 0], [4, 0, 0]], one, 4.0),       # two corners in one place, 4
        ("twice", [[1, 1, 2], [9, 9, 9]], RIGHT, [[0, 1, 2], [0, 1, 2]], 4.0),          # the lower index; and a point beyond
    ]
    return [(name, np.asarray(p, np.float32), np.asarray(v, np.float32), np.asarray(t, np.int64), D) for name, p, v, t, D in out]


HAND_ANSWERS = dict(interior=4.0, edge=25.0, corner=9.0, on_plane=0.0, collinear=4.0, coincident=4.0)


def fan(num_triangles, seed=0):
    """A fan of triangles around one vertex inside the unit cube: every triangle's box holds the centre."""
    rng = np.random.default_rng(seed)
    v = np.concatenate([[[0.5, 0.5, 0.5]], rng.uniform(0, 1, (num_triangles + 1, 3))]).astype(np.float32)
    k = np.arange(num_triangles)
    return v, np.stack([np.zeros(num_triangles, np.int64), 1 + k, 2 + k], axis=1)


def sprinkled(tri, num_vertices, seed=0, every=7):
    """tri with an index V, an index 0xFFFFFFFF and a vertex twice put into every `every`-th triangle in turn."""
    t = np.asarray(tri, np.int64).copy()
    rows = np.arange(0, len(t), every)
    t[rows[0::3], 1] = num_vertices
    t[rows[1::3], 2] = 0xFFFFFFFF
    t[rows[2::3], 0] = t[rows[2::3], 1]
    return t
