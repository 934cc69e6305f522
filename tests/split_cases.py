"""A CPU oracle for the long-edge split (mlsgpu_hip_mesh_split_edges), and the meshes its tests share.

split() follows the contract in include/mlsgpu_hip.h step by step, a round at a time: the directed sides of the participating
triangles are sorted once per round (np.unique), an edge's two directions and a triangle's first side are looked up in the
sorted arrays, and float64 arrays hold the lengths -- every numpy operation is one correctly rounded double operation, written
in the contract's order.  Nothing here is product code.
"""
import numpy as np

from flip_cases import Invalid, classes, defect_mesh, dot, flat_grid, grid_mesh, quality, triangle_set  # noqa: F401  (the tests use them)
from normals_cases import fan_mesh  # noqa: F401
from smooth_cases import noisy_torus  # noqa: F401

STAT_NAMES = ("numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "numEdges", "interiorEdges",
              "boundaryEdges", "rounds", "splits", "boundarySplits", "converged", "limited", "longBefore", "longAfter",
              "blockedAfter", "outVertices", "outTriangles", "minQualityBefore", "minQualityAfter", "maxLengthSqBefore",
              "maxLengthSqAfter", "qualityBefore", "qualityAfter")
QUALITY_NAMES = ("minQualityBefore", "minQualityAfter", "qualityBefore", "qualityAfter")
U32 = np.uint64(32)
LOW = np.uint64(0xFFFFFFFF)
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def empty_stats():
    out = dict.fromkeys(STAT_NAMES, 0)
    out.update(minQualityBefore=0.0, minQualityAfter=0.0, maxLengthSqBefore=0.0, maxLengthSqAfter=0.0, qualityBefore=[0] * 16,
               qualityAfter=[0] * 16)
    return out


def classify(p, tri, live, limit, pinned):
    """Steps 2 to 6 on the current triangles: the counts, and per candidate, in ascending (a, b): a, b, and for T1 and T2 the
    row, the corner that holds b and the third vertex (row -1 where the edge has no such triangle)."""
    slots = np.flatnonzero(live)
    t = tri[live]
    n = len(t)
    src, dst, opp = t.ravel().astype(np.uint64), t[:, [1, 2, 0]].ravel().astype(np.uint64), t[:, [2, 0, 1]].ravel()
    slot, corner = np.repeat(slots, 3), np.tile(np.arange(3), n)
    sides, first, uses = np.unique(src << U32 | dst, return_index=True, return_counts=True)        # the round's one sort
    pair = np.minimum(src, dst) << U32 | np.maximum(src, dst)
    edges = np.unique(pair)
    a, b = edges >> U32, edges & LOW
    counts = dict(numEdges=len(edges), interiorEdges=0, boundaryEdges=0, long=0, blocked=0, maxLengthSq=0.0)
    if n == 0:
        return counts, None

    def found(key):
        at = np.minimum(np.searchsorted(sides, key), len(sides) - 1)
        has = sides[at] == key
        return first[at], np.where(has, uses[at], 0)

    r1, up = found(a << U32 | b)                                # the record of a -> b in T1, and how many sides are a -> b
    r2, down = found(b << U32 | a)
    ai, bi = a.astype(np.int64), b.astype(np.int64)
    interior = (up == 1) & (down == 1) & (opp[r1] != opp[r2])   # step 2
    boundary = up + down == 1
    e = p[bi] - p[ai]
    L2 = dot(e, e)                                              # step 3
    long_ = L2 > limit
    splittable = long_ & (interior | boundary) & ~(pinned[ai] & pinned[bi])        # step 4
    # step 5: every triangle's first side, by its own three lengths
    s, d = src.astype(np.int64), dst.astype(np.int64)
    es = p[d] - p[s]
    side_l2 = dot(es, es).reshape(n, 3)
    ties = np.where(side_l2 == side_l2.max(axis=1)[:, None], pair.reshape(n, 3), NONE)
    first_of = ties.min(axis=1)                                 # per live triangle: the pair of its first side
    cand = splittable & ((up != 1) | (first_of[r1 // 3] == edges)) & ((down != 1) | (first_of[r2 // 3] == edges))  # step 6
    counts.update(interiorEdges=int(interior.sum()), boundaryEdges=int(boundary.sum()), long=int(long_.sum()),
                  blocked=int((long_ & ~splittable).sum()), maxLengthSq=float(L2.max()))
    k = np.flatnonzero(cand)
    has1, has2 = up[k] == 1, down[k] == 1
    return counts, dict(a=ai[k], b=bi[k], boundary=boundary[k],
                        row1=np.where(has1, slot[r1[k]], -1), corner1=(corner[r1[k]] + 1) % 3, c=opp[r1[k]],
                        row2=np.where(has2, slot[r2[k]], -1), corner2=corner[r2[k]], d=opp[r2[k]])


def split(vertices, triangles, max_rounds, max_length, max_out_triangles=0, pinned=None):
    """(vertices float32 [V', 3], triangles uint32 [T', 3], statistics dict, ends uint32 [V' - V, 2]) or Invalid."""
    p32 = np.array(vertices, np.float32).reshape(-1, 3)
    tri = np.array(triangles, np.int64).reshape(-1, 3) & 0xFFFFFFFF
    V, T = len(p32), len(tri)
    if not (np.isfinite(max_length) and max_length > 0 and (max_out_triangles == 0 or max_out_triangles >= T)):
        raise Invalid("parameters")
    if not np.isfinite(p32).all():
        raise Invalid("vertex")
    pin = np.zeros(V, bool) if pinned is None else np.array(pinned, np.uint8).reshape(V) != 0
    limit = np.float64(max_length) * np.float64(max_length)
    p = p32.astype(np.float64)
    stats = empty_stats()
    stats.update(numVertices=V, numTriangles=T)
    out_of_range, degenerate = classes(V, tri)                  # step 1: of the input, once
    live = ~out_of_range & ~degenerate
    stats.update(outOfRangeTriangles=int(out_of_range.sum()), degenerateTriangles=int(degenerate.sum()))
    stats["minQualityBefore"], stats["qualityBefore"] = quality(p, tri, live)
    ends = np.zeros((0, 2), np.uint32)
    first = True
    while True:                                                 # step 8
        counts, c = classify(p, tri, live, limit, pin)
        if first:
            stats.update(numEdges=counts["numEdges"], interiorEdges=counts["interiorEdges"], boundaryEdges=counts["boundaryEdges"],
                         longBefore=counts["long"], maxLengthSqBefore=counts["maxLengthSq"])
            first = False
        stats.update(longAfter=counts["long"], blockedAfter=counts["blocked"], maxLengthSqAfter=counts["maxLengthSq"])
        if stats["rounds"] == max_rounds:
            break
        n = len(c["a"]) if c is not None else 0
        if n == 0:
            stats["rounds"] += 1
            stats["converged"] = 1
            break
        has1, has2 = c["row1"] >= 0, c["row2"] >= 0
        rows = has1.astype(np.int64) + has2
        new_v, new_t = len(p32) + n, len(tri) + int(rows.sum())
        if (max_out_triangles != 0 and new_t > max_out_triangles) or new_v >= 2 ** 32 or 3 * new_t >= 2 ** 32:
            stats["limited"] = 1
            break
        stats["rounds"] += 1
        stats["splits"] += n
        stats["boundarySplits"] += int(c["boundary"].sum())
        a, b = c["a"], c["b"]                                   # step 7
        m = len(p32) + np.arange(n)
        at = len(tri) + np.cumsum(rows) - rows
        middle = ((p[a] + p[b]) * 0.5).astype(np.float32)
        tri = np.concatenate([tri, np.zeros((int(rows.sum()), 3), np.int64)])
        tri[c["row1"][has1], c["corner1"][has1]] = m[has1]
        tri[c["row2"][has2], c["corner2"][has2]] = m[has2]
        tri[at[has1]] = np.stack([m, b, c["c"]], axis=1)[has1]
        tri[(at + has1)[has2]] = np.stack([b, m, c["d"]], axis=1)[has2]
        live = np.concatenate([live, np.ones(int(rows.sum()), bool)])
        p32 = np.concatenate([p32, middle])
        pin = np.concatenate([pin, np.zeros(n, bool)])
        ends = np.concatenate([ends, np.stack([a, b], axis=1).astype(np.uint32)])
        p = p32.astype(np.float64)
    stats["minQualityAfter"], stats["qualityAfter"] = quality(p, tri, live)
    stats.update(outVertices=len(p32), outTriangles=len(tri))
    return p32, tri.astype(np.uint32), stats, ends


def assert_same(got, want):
    """(vertices, triangles, stats[, ends]) against the oracle's: every bit, every row and every statistic exactly."""
    assert got[2] == want[2], (got[2], want[2])
    gv, wv = np.ascontiguousarray(got[0], np.float32).reshape(-1, 3), np.ascontiguousarray(want[0], np.float32).reshape(-1, 3)
    assert gv.shape == wv.shape and gv.tobytes() == wv.tobytes()
    gt = np.ascontiguousarray(got[1], np.uint32).reshape(-1, 3)
    assert gt.shape == want[1].shape
    np.testing.assert_array_equal(gt, want[1])
    if len(got) > 3:
        ge = np.asarray(got[3], np.uint32).reshape(-1, 2)
        assert ge.shape == want[3].shape
        np.testing.assert_array_equal(ge, want[3])


def invariants(num_vertices, triangles):
    """What a split keeps of topology_cases.count_all's report, and the boundary edges, which rise by boundarySplits."""
    import topology_cases as tc
    r = tc.count_all(num_vertices, np.asarray(triangles, np.int64).reshape(-1, 3))
    return dict((name, r[name]) for name in ("manifold", "numComponents", "numBoundaries", "eulerCharacteristic", "boundaryEdges"))


def area(vertices, triangles):
    p, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    return float(np.linalg.norm(np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]), axis=1).sum() / 2)


def longest_edge(vertices, triangles):
    p, t = np.asarray(vertices, np.float64), np.asarray(triangles, np.int64)
    return float(np.sqrt(max(dot(p[t[:, k]] - p[t[:, (k + 1) % 3]], p[t[:, k]] - p[t[:, (k + 1) % 3]]).max() for k in range(3))))


def rim_of(num_vertices, triangles):
    """One byte per vertex: 1 on a boundary edge."""
    t = np.asarray(triangles, np.int64)
    a, b = t.ravel(), t[:, [1, 2, 0]].ravel()
    sides = set(zip(a.tolist(), b.tolist()))
    pinned = np.zeros(num_vertices, np.uint8)
    for x, y in sides:
        if (y, x) not in sides:
            pinned[x] = pinned[y] = 1
    return pinned


def rotated(triangles, seed):
    t = np.asarray(triangles)
    turns = np.random.default_rng(seed).integers(0, 3, len(t))
    return np.stack([t[np.arange(len(t)), (turns + k) % 3] for k in range(3)], axis=1)


# ---------------------------------------------------------------- meshes

def one_triangle():
    """Sides 0 1 of length 4, 1 2 of length sqrt 10, 2 0 of length sqrt 2: at maxLength 3.5 only 0 1 is split."""
    return np.array([[0, 0, 0], [4, 0, 0], [1, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int64)


def long_diagonal():
    """A square whose diagonal 0 1 (length sqrt 8) is its only edge above 2.5."""
    p = np.array([[0, 0, 0], [2, 2, 0], [0, 2, 0], [2, 0, 0]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 3]], np.int64)


def tied_pair():
    """The two right isosceles triangles of an unjittered grid cell, and the lower half of the next cell: vertices 0..4 at
    (0,0) (1,0) (0,1) (1,1) (2,0).  In every triangle the two legs tie, behind the hypotenuse."""
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 0, 0]], np.float32)
    return p, np.array([[0, 1, 2], [1, 3, 2], [1, 4, 3]], np.int64)


def isosceles():
    """One triangle whose two longest sides tie: 0 2 and 1 2 have L2 = 10, and (0, 2) < (1, 2) makes 0 2 the first side."""
    return np.array([[0, 0, 0], [2, 0, 0], [1, 3, 0]], np.float32), np.array([[0, 1, 2]], np.int64)


def fin():
    """Three triangles on the edge 0 1, which is the longest side of each."""
    p = np.array([[0, 0, 0], [4, 0, 0], [2, 1, 0], [2, -1, 0], [2, 0, 1]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int64)
