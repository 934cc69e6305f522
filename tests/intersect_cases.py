"""A CPU oracle for the self-intersection report (mlsgpu_hip_mesh_self_intersections), and what its tests share.

self_intersections() follows the contract in include/mlsgpu_hip.h step by step, with explicit element-wise float64 operations
in the contract's order (no np.dot, einsum, np.cross or linalg: their summation order is not the contract's).  The candidates of
step 2 come by one of two routes that must agree: brute force over all pairs of participating triangles (below BRUTE_BELOW
triangles), or a numpy grid of the oracle's own, in which a pair is looked at only in the cell that holds the larger of the
two boxes' lower corners -- step 2 is then applied exactly to what the grid hands over, as the contract allows any
conservative cull to do.  Every orient() is a pure function of its twelve coordinates, so the oracle evaluates the three side
signs of step 4 only where the plane signs differ: what it leaves out cannot change a result.  Nothing here is product code.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

STAT_NAMES = ("numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "candidatePairs", "crossingPairs",
              "crossingTriangles", "lowestA", "lowestB", "maxPartners", "maxPartnersTriangle", "lowestChunk", "crossingChunks")
NONE = 2 ** 64 - 1
BRUTE_BELOW = 2000              # triangles: below this, brute force
BLOCK_PAIRS = 1 << 19           # pairs looked at at a time
PREDICATE_PAIRS = 1 << 14       # pairs that steps 3 to 5 are worked out for at a time
THREADS = min(16, os.cpu_count() or 1)
GRID_PAIRS = 1 << 23            # (cell, triangle) records the oracle's grid may hold
FILTER = 2.0 ** -48             # step 3


class Invalid(Exception):
    """What the device reports as MLSGPU_ERR_INVALID."""


# ---------------------------------------------------------------- step 3, on tuples (x, y, z) of float64 arrays [N]

def _sub(u, v):
    return u[0] - v[0], u[1] - v[1], u[2] - v[2]


def orient(a, b, c, x):
    """The certain sign of step 3 for N point quadruples: int8 [N], -1, 0 or +1."""
    r0, r1, r2 = _sub(a, x), _sub(b, x), _sub(c, x)
    yz, zy = r1[1] * r2[2], r1[2] * r2[1]
    zx, xz = r1[2] * r2[0], r1[0] * r2[2]
    xy, yx = r1[0] * r2[1], r1[1] * r2[0]
    det = (r0[0] * (yz - zy) + r0[1] * (zx - xz)) + r0[2] * (xy - yx)
    perm = (np.abs(r0[0]) * (np.abs(yz) + np.abs(zy)) + np.abs(r0[1]) * (np.abs(zx) + np.abs(xz))) \
        + np.abs(r0[2]) * (np.abs(xy) + np.abs(yx))
    return np.where(np.abs(det) <= perm * FILTER, 0, np.sign(det)).astype(np.int8)


def _points(corners, k, rows=None):
    """Corner k of triangles given as float64 [N, 3 corners, 3 axes], as a tuple of coordinate arrays."""
    c = corners[:, k] if rows is None else corners[rows, k]
    return c[:, 0], c[:, 1], c[:, 2]


def _pierced_by(S, T):
    """Steps 4 and 5, one direction: which of the N triangles T are pierced by a side of S, in S's stored corner order."""
    t = [_points(T, k) for k in range(3)]
    side_of = [orient(t[0], t[1], t[2], _points(S, k)) for k in range(3)]
    hit = np.zeros(len(S), bool)
    for k in range(3):
        rows = np.flatnonzero(side_of[k].astype(np.int16) * side_of[(k + 1) % 3] < 0)
        if len(rows) == 0:
            continue
        p, q = _points(S, k, rows), _points(S, (k + 1) % 3, rows)
        a, b, c = (_points(T, j, rows) for j in range(3))
        s0, s1, s2 = orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a)
        hit[rows[(s0 != 0) & (s0 == s1) & (s1 == s2)]] = True
    return hit


def crosses(A, B):
    """Step 5 for N pairs of triangles given as corner arrays [N, 3, 3] (float32 or float64): a mask."""
    A, B = np.asarray(A, np.float64).reshape(-1, 3, 3), np.asarray(B, np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        return _pierced_by(A, B) | _pierced_by(B, A)


# ---------------------------------------------------------------- steps 1 and 2

def participating(num_vertices, triangles):
    """Step 1: (the indices of the triangles that take part, outOfRangeTriangles, degenerateTriangles)."""
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    bad = ((tri >= int(num_vertices)) | (tri < 0)).any(axis=1)
    degenerate = ~bad & ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0]))
    return np.flatnonzero(~bad & ~degenerate), int(bad.sum()), int(degenerate.sum())


def _overlap(lo, hi, i, j):
    """Step 2 for the pairs of positions (i[k], j[k]): float comparisons of the boxes' corners."""
    return ((lo[i] <= hi[j]) & (lo[j] <= hi[i])).all(axis=1)


def _brute_blocks(n):
    """All pairs i < j of n positions as jobs: each expands a range of rows i into its pairs."""
    rows = max(1, BLOCK_PAIRS // max(n, 1))

    def expand(first, last):
        i = np.repeat(np.arange(first, last, dtype=np.int64), n)
        j = np.tile(np.arange(n, dtype=np.int64), last - first)
        keep = i < j
        return i[keep], j[keep]
    return [(expand, first, min(n, first + rows)) for first in range(0, n, rows)]


def _grid_blocks(lo, hi):
    """A superset of the candidates, every candidate exactly once: a triangle goes into every cell from cell(lo) to cell(hi),
    cell() monotone, so two overlapping boxes share the cell max(cell(loA), cell(loB)) per axis, and a pair is handed over
    only from there.  Jobs that each expand a range of (cell, triangle) records into pairs of positions (i, j) with i < j."""
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    origin, top = lo64.min(axis=0), hi64.max(axis=0)
    g = float(np.mean((hi64 - lo64).max(axis=1)))
    if not g > 0.0:
        g = 1.0
    while True:
        n = np.maximum(np.floor((top - origin) / g).astype(np.int64) + 1, 1)

        def cell(x):
            return np.clip(np.floor((x - origin) / g), 0, n - 1).astype(np.int64)
        c0, c1 = cell(lo64), cell(hi64)
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
    here = np.stack([x[order], y[order], z[order]], axis=1)
    # record r pairs with the later records of its cell's run
    length = np.searchsorted(key, key, "right") - np.arange(len(key)) - 1
    ends = np.cumsum(length)

    def expand(at, upto):
        rows = np.arange(at, upto, dtype=np.int64)
        ri = np.repeat(rows, length[rows])
        rj = ri + 1 + np.arange(len(ri), dtype=np.int64) - np.repeat(np.cumsum(length[rows]) - length[rows], length[rows])
        i, j = owner[ri], owner[rj]
        own = (np.maximum(c0[i], c0[j]) == here[ri]).all(axis=1)
        i, j = i[own], j[own]
        return np.minimum(i, j), np.maximum(i, j)
    jobs, at = [], 0
    while at < len(key):
        upto = max(at + 1, int(np.searchsorted(ends, (ends[at - 1] if at else 0) + BLOCK_PAIRS, "right")))
        jobs.append((expand, at, upto))
        at = upto
    return jobs


def self_intersections(vertices, triangles, prune=None):
    """(partners uint32 [T], pairs uint32 [crossingPairs, 2] sorted, statistics dict) or Invalid.  prune: True / False forces
    the grid or brute force; None chooses by the number of triangles."""
    vf = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    if not np.isfinite(vf).all():
        raise Invalid("vertex")
    V, T = len(vf), len(tri)
    live, bad, degenerate = participating(V, tri)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats.update(numVertices=V, numTriangles=T, outOfRangeTriangles=bad, degenerateTriangles=degenerate, lowestA=NONE, lowestB=NONE,
                 maxPartnersTriangle=NONE)
    partners = np.zeros(T, np.int64)
    found = [np.zeros((0, 2), np.int64)]
    if len(live) > 1:
        corners = vf[tri[live]]                                 # [n, 3 corners, 3 axes]
        lo, hi = corners.min(axis=1), corners.max(axis=1)       # float32
        wide = corners.astype(np.float64)
        if prune is None:
            prune = len(live) >= BRUTE_BELOW

        def work(job):
            expand, first, last = job
            i, j = expand(first, last)
            keep = _overlap(lo, hi, i, j)
            i, j = i[keep], j[keep]
            hit = np.zeros(len(i), bool)
            for at in range(0, len(i), PREDICATE_PAIRS):        # in pieces whose temporaries stay in the cache
                piece = slice(at, at + PREDICATE_PAIRS)
                hit[piece] = crosses(wide[i[piece]], wide[j[piece]])
            return len(i), np.stack([live[i[hit]], live[j[hit]]], axis=1)
        # the blocks are independent and numpy drops the lock while it works: threads only shorten the wait
        with ThreadPoolExecutor(THREADS) as pool:
            for candidates, crossing in pool.map(work, _grid_blocks(lo, hi) if prune else _brute_blocks(len(live))):
                stats["candidatePairs"] += candidates
                found.append(crossing)
    pairs = np.concatenate(found)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    assert len(np.unique(pairs, axis=0)) == len(pairs) and (pairs[:, 0] < pairs[:, 1]).all()
    np.add.at(partners, pairs.ravel(), 1)
    stats["crossingPairs"] = len(pairs)
    stats["crossingTriangles"] = int((partners > 0).sum())
    if len(pairs):
        stats.update(lowestA=int(pairs[0, 0]), lowestB=int(pairs[0, 1]), maxPartners=int(partners.max()),
                     maxPartnersTriangle=int(np.argmax(partners)))
    return partners.astype(np.uint32), pairs.astype(np.uint32), stats


def combined(reports):
    """The reports of a sink's dense chunks, in chunk order, as mlsgpu_hip_mesher_self_intersections adds them up."""
    total = dict.fromkeys(STAT_NAMES, 0)
    total.update(lowestA=NONE, lowestB=NONE, maxPartnersTriangle=NONE)
    for c, one in enumerate(reports):
        for name in ("numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "candidatePairs", "crossingPairs",
                     "crossingTriangles"):
            total[name] += one[name]
        if one["crossingPairs"] > 0:
            if total["crossingChunks"] == 0:
                total.update(lowestChunk=c, lowestA=one["lowestA"], lowestB=one["lowestB"])
            total["crossingChunks"] += 1
            if one["maxPartners"] > total["maxPartners"]:
                total.update(maxPartners=one["maxPartners"], maxPartnersTriangle=one["maxPartnersTriangle"])
    return total


def same_stats(got, want):
    """The report's fields (a dict from the binding may hold others besides)."""
    g, w = dict((k, got[k]) for k in STAT_NAMES), dict((k, want[k]) for k in STAT_NAMES)
    assert g == w, (g, w)


def assert_same(got, want):
    """(partners, pairs, stats) against the oracle's, exactly.  A None among got's arrays (an output the caller did not take)
    is not compared."""
    gp, gl, gs = got
    wp, wl, ws = want
    same_stats(gs, ws)
    if gp is not None:
        np.testing.assert_array_equal(np.asarray(gp, np.uint32), np.asarray(wp, np.uint32))
    if gl is not None:
        np.testing.assert_array_equal(np.asarray(gl, np.uint32).reshape(-1, 2), np.asarray(wl, np.uint32).reshape(-1, 2))


# ---------------------------------------------------------------- hand cases: (name, vertices, triangles, crossing pairs)

def hand_cases():
    flat = [[0, 0, 0], [4, 0, 0], [0, 4, 0]]
    two = [[0, 1, 2], [3, 4, 5]]
    out = [
        # two triangles through each other's middle: a side of each pierces the other
        ("plus", [[-2, 0, -1], [2, 0, -1], [0, 0, 3], [0, -2, 1], [0, 2, 1], [0, 0, -3]], two, 1),
        # a tip through the face: the two sides at the tip pierce it
        ("tip", flat + [[1, 1, -1], [1.5, 1, 3], [1, 1.5, 3]], two, 1),
        ("touch_point", flat + [[1, 1, 0], [1, 1, 3], [2, 1, 3]], two, 0),             # a corner rests on the face
        ("touch_side", flat + [[1, 1, 0], [2, 1, 0], [1, 1, 3]], two, 0),              # a side rests on the face
        ("coplanar", flat + [[1, 1, 0], [5, 1, 0], [1, 5, 0]], two, 0),                # overlap in one plane
        # corner 0 shared, and the side opposite to it goes through the other face
        ("shared_corner", flat + [[1, 1, -1], [1, 1, 1]], [[0, 1, 2], [0, 3, 4]], 1),
        ("shared_side", flat + [[0, 0, 3]], [[0, 1, 2], [1, 0, 3]], 0),
        ("twice", flat, [[0, 1, 2], [0, 1, 2]], 0),
    ]
    return [(name, np.asarray(v, np.float32), np.asarray(t, np.int64), n) for name, v, t, n in out]


def needles(count, seed=0):
    """`count` long thin triangles through the centre of the unit cube, each with its own three vertices."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(count, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    centre = 0.5 + rng.uniform(-0.02, 0.02, (count, 3))
    w = np.cross(d, rng.normal(size=(count, 3)))
    w *= 0.01 / np.sqrt((w * w).sum(axis=1))[:, None]
    v = np.stack([centre - 2.0 * d, centre + 2.0 * d + w, centre + 2.0 * d - w], axis=1).reshape(-1, 3).astype(np.float32)
    return v, np.arange(3 * count, dtype=np.int64).reshape(-1, 3)


def joined(*meshes):
    """Meshes (vertices, triangles) as one, each with its own vertices."""
    v, t, base = [], [], 0
    for p, tri in meshes:
        v.append(np.asarray(p, np.float32))
        t.append(np.asarray(tri, np.int64) + base)
        base += len(p)
    return np.concatenate(v), np.concatenate(t)


def tilted(p, slope=0.5, about=19.37):
    """p with z replaced by z + slope * (x - about), in float32."""
    q = np.asarray(p, np.float32).copy()
    q[:, 2] = q[:, 2] + np.float32(slope) * (q[:, 0] - np.float32(about))
    return q
