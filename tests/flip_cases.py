"""A CPU oracle for the Delaunay edge flips (mlsgpu_hip_mesh_flip_edges), and the meshes its tests share.

flip() follows the contract in include/mlsgpu_hip.h step by step, a round at a time over sorted side arrays: np.unique on the
directed sides for the runs, np.searchsorted for a side's reverse and for guard (i), float64 arrays for P, the guards and the
quality -- every numpy operation is one correctly rounded double operation, written in the contract's order --, and
np.maximum.at / np.minimum.at for the choice of a round.  Nothing here is product code.
"""
import numpy as np

from simplify_cases import grid_mesh, torus_mesh  # noqa: F401  (the tests take their meshes from here)

MIN_GAIN, MIN_COS = 1e-6, 0.5
TWO_ROOT_THREE = 3.4641016151377544
STAT_NAMES = ("numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "numEdges", "interiorEdges", "rounds",
              "flips", "converged", "nonDelaunayBefore", "nonDelaunayAfter", "blockedAfter", "minQualityBefore", "minQualityAfter",
              "qualityBefore", "qualityAfter")
U32 = np.uint64(32)


class Invalid(Exception):
    """What the device reports as MLSGPU_ERR_INVALID."""


def empty_stats():
    out = dict.fromkeys(STAT_NAMES, 0)
    out.update(minQualityBefore=0.0, minQualityAfter=0.0, qualityBefore=[0] * 16, qualityAfter=[0] * 16)
    return out


# ---------------------------------------------------------------- the contract's vector operations, on [n, 3] float64 arrays

def dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                     u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def face(p, q, r):
    return cross(q - p, r - p)


def cot(p, q, r):
    x = cross(q - p, r - p)
    with np.errstate(divide="ignore", invalid="ignore"):
        return dot(q - p, r - p) / np.sqrt(dot(x, x))


def classes(num_vertices, tri):
    """Step 1: (out of range, degenerate) masks."""
    bad = ((tri >= num_vertices) | (tri < 0)).any(axis=1)
    return bad, ~bad & ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0]))


def quality(p, tri, live):
    """Step 9: (the smallest q, the histogram) of the participating triangles."""
    t = tri[live]
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    x, u, v, w = face(a, b, c), b - a, c - b, a - c
    denominator = (dot(u, u) + dot(v, v)) + dot(w, w)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (TWO_ROOT_THREE * np.sqrt(dot(x, x))) / denominator
    q[(denominator == 0) | np.isnan(q)] = 0.0
    bins = np.minimum(15, np.floor(16.0 * q)).astype(np.int64)
    return (float(q.min()) if len(q) else 0.0), np.bincount(bins, minlength=16).tolist()


def classify(p, tri, live, min_gain, min_cos):
    """Steps 2 to 5 on the current triangles: the counts, and per candidate a, b, c, d, P, the slots of T1 and T2."""
    slots = np.flatnonzero(live)
    t = tri[live]
    src, dst, opp = t.ravel().astype(np.uint64), t[:, [1, 2, 0]].ravel().astype(np.uint64), t[:, [2, 0, 1]].ravel()
    slot = np.repeat(slots, 3)
    key = src << U32 | dst
    sides, first, uses = np.unique(key, return_index=True, return_counts=True)
    num_edges = len(np.unique(np.minimum(src, dst) << U32 | np.maximum(src, dst)))
    a, b = sides >> U32, sides & np.uint64(0xFFFFFFFF)
    back = np.searchsorted(sides, b << U32 | a)
    back[back == len(sides)] = 0
    regular = (a < b) & (uses == 1) & (sides[back] == (b << U32 | a)) & (uses[back] == 1) if len(sides) else np.zeros(0, bool)
    i, j = first[regular], first[back[regular]]
    a, b, c, d = a[regular].astype(np.int64), b[regular].astype(np.int64), opp[i], opp[j]
    keep = c != d                                               # step 3
    a, b, c, d, t1, t2 = a[keep], b[keep], c[keep], d[keep], slot[i][keep], slot[j][keep]
    pa, pb, pc, pd = p[a], p[b], p[c], p[d]
    with np.errstate(invalid="ignore"):
        P = -(cot(pc, pa, pb) + cot(pd, pb, pa))                # step 4
        bad = P > min_gain
    n1, n2, m1, m2 = face(pa, pb, pc), face(pb, pa, pd), face(pa, pd, pc), face(pb, pc, pd)
    N = n1 + n2
    with np.errstate(invalid="ignore"):
        flat = dot(n1, n2) >= (min_cos * np.sqrt(dot(n1, n1))) * np.sqrt(dot(n2, n2))
        convex = (dot(m1, N) > 0) & (dot(m2, N) > 0)
    cu, du = c.astype(np.uint64), d.astype(np.uint64)
    taken = np.isin(cu << U32 | du, sides) | np.isin(du << U32 | cu, sides)
    cand = bad & flat & convex & ~taken
    counts = dict(numEdges=num_edges, interiorEdges=int(keep.sum()), nonDelaunay=int(bad.sum()), blocked=int((bad & ~cand).sum()))
    return counts, [x[cand] for x in (a, b, c, d, P, t1, t2)]


def winners(num_vertices, a, b, c, d, P):
    """Step 6: the mask of the candidates that win."""
    key = a.astype(np.uint64) << U32 | b.astype(np.uint64)     # ordered as a << bitLength(V) | b is
    best = np.full(num_vertices, -np.inf)
    for v in (a, b, c, d):
        np.maximum.at(best, v, P)
    least = np.full(num_vertices, np.iinfo(np.uint64).max, np.uint64)
    for v in (a, b, c, d):
        holds = P == best[v]
        np.minimum.at(least, v[holds], key[holds])
    win = np.ones(len(P), bool)
    for v in (a, b, c, d):
        win &= (P == best[v]) & (key == least[v])
    return win


def flip(vertices, triangles, max_rounds, min_gain=MIN_GAIN, min_cos=MIN_COS, trace=None):
    """(triangles uint32 [T, 3], statistics dict) or Invalid.  `trace`, a list, gets one dict per round: its candidates, its
    winners, and whether two of its candidates have the same P."""
    p32 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.array(triangles, np.int64).reshape(-1, 3) & 0xFFFFFFFF
    if not (np.isfinite(min_gain) and min_gain >= 0 and -1 <= min_cos <= 1):
        raise Invalid("parameters")
    if not np.isfinite(p32).all():
        raise Invalid("vertex")
    p, V = p32.astype(np.float64), len(p32)
    stats = empty_stats()
    stats.update(numVertices=V, numTriangles=len(tri))
    out_of_range, degenerate = classes(V, tri)
    live = ~out_of_range & ~degenerate
    stats.update(outOfRangeTriangles=int(out_of_range.sum()), degenerateTriangles=int(degenerate.sum()))
    stats["minQualityBefore"], stats["qualityBefore"] = quality(p, tri, live)
    first = True
    while True:                                                 # step 8
        counts, (a, b, c, d, P, t1, t2) = classify(p, tri, live, min_gain, min_cos)
        if first:
            stats.update(numEdges=counts["numEdges"], interiorEdges=counts["interiorEdges"], nonDelaunayBefore=counts["nonDelaunay"])
            first = False
        stats.update(nonDelaunayAfter=counts["nonDelaunay"], blockedAfter=counts["blocked"])
        if stats["rounds"] == max_rounds:
            break
        stats["rounds"] += 1
        win = winners(V, a, b, c, d, P)
        if trace is not None:
            trace.append(dict(candidates=len(P), winners=int(win.sum()), ties=len(np.unique(P)) != len(P)))
        assert win.any() == (len(P) > 0)
        if not win.any():
            stats["converged"] = 1
            break
        stats["flips"] += int(win.sum())
        tri[t1[win]] = np.stack([a, d, c], axis=1)[win]         # step 7
        tri[t2[win]] = np.stack([b, c, d], axis=1)[win]
    stats["minQualityAfter"], stats["qualityAfter"] = quality(p, tri, live)
    return tri.astype(np.uint32), stats


def assert_same(got, want):
    """(triangles, stats) against the oracle's: every row and every statistic exactly."""
    gt, gs = got
    wt, ws = want
    assert gs == ws, (gs, ws)
    gt = np.ascontiguousarray(gt, np.uint32).reshape(-1, 3)
    assert gt.shape == wt.shape
    np.testing.assert_array_equal(gt, wt)


def triangle_set(tri):
    """The triangles up to rotation: sorted rows that start at their smallest index."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    k = np.argmin(tri, axis=1)
    rows = np.stack([tri[np.arange(len(tri)), (k + s) % 3] for s in range(3)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def edge_set(tri, num_vertices):
    """The undirected edges of the participating triangles, as sorted codes."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3) & 0xFFFFFFFF
    bad, degenerate = classes(num_vertices, tri)
    t = tri[~bad & ~degenerate]
    lo, hi = np.minimum(t, t[:, [1, 2, 0]]).ravel(), np.maximum(t, t[:, [1, 2, 0]]).ravel()
    return np.unique(lo << 32 | hi)


# ---------------------------------------------------------------- meshes

def kite():
    """A thin kite: a = 0 and b = 1 far apart, c = 2 and d = 3 close to the middle of a b.  Both angles opposite a b are
    obtuse: it flips to (a, d, c), (b, c, d)."""
    p = np.array([[-4, 0, 0], [4, 0, 0], [0, 1, 0], [0, -1, 0]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 3]], np.int64)


def square():
    """The unit square cut along a diagonal: its corners lie on one circle, both opposite angles are right, P == 0."""
    p = np.array([[0, 0, 0], [1, 1, 0], [0, 1, 0], [1, 0, 0]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 3]], np.int64)


def tetrahedron():
    """A flat closed tetrahedron: the apex 3 barely above the obtuse triangle 0 1 2.  Edge 0 1 is non-Delaunay, and the edge
    2 3 its flip would make is there already."""
    p = np.array([[-4, 0, 0], [4, 0, 0], [0, 1, 0], [0, -1, 0.25]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 3], [1, 3, 2], [3, 0, 2]], np.int64)


def pillow():
    """Two triangles over the same three vertices, back to back: every edge has c == d."""
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 2]], np.int64)


def folded():
    """The kite with d turned up by 90 degrees around a b."""
    p = np.array([[-4, 0, 0], [4, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 3]], np.int64)


def concave():
    """A dart: T2 is folded over onto c's side of a b, with d = 3 beside c, so the quad a d b c is not convex and the flip
    would leave (b, c, d) upside down.  Both opposite angles are obtuse; n1 = 8 z, n2 = -4 z: guard (ii) holds with equality
    at minCos -1, and m2 . N = -4.  (In a plane, two triangles that face the same way and have P > 0 always make a convex quad:
    the angles at c and d sum to more than pi, so those at a and b sum to less.)"""
    p = np.array([[-4, 0, 0], [4, 0, 0], [0, 1, 0], [3, 0.5, 0]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 3]], np.int64)


def cap():
    """T1 has no area: c = 2 lies on a b.  cot at c is -infinity, P is +infinity, and the long edge flips."""
    p = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [1, -1, 0]], np.float32)
    return p, np.array([[0, 1, 2], [1, 0, 3]], np.int64)


def flat_grid(n, m, jitter, seed):
    """grid_mesh(n, m) with x and y of every vertex moved by up to `jitter` (seeded) and z = 0."""
    p, tri = grid_mesh(n, m)
    p = p.astype(np.float64)
    p[:, :2] += np.random.default_rng(seed).uniform(-jitter, jitter, (len(p), 2))
    return p.astype(np.float32), tri


def defect_mesh():
    """A jittered flat grid with a triangle that names vertex 0xFFFFFFFF, one that names V, two degenerate triangles and two
    unused vertices."""
    p, tri = flat_grid(9, 11, 0.3, 3)
    p = np.concatenate([p, [[4.0, 4.0, 1.0], [-2.0, 0.5, 0.25]]]).astype(np.float32)
    tri = tri.copy()
    tri[5, 2] = len(p)
    tri[77, 0] = 0xFFFFFFFF
    tri[20, 1] = tri[20, 0]
    tri[121, 2] = tri[121, 1]
    return p, tri


def renumbered(p, tri, seed):
    """The same mesh with its vertices in another order: (vertices, triangles, perm) with new vertex perm[v] = old vertex v."""
    perm = np.random.default_rng(seed).permutation(len(p))
    q = np.empty_like(p)
    q[perm] = p
    return q, perm[np.asarray(tri, np.int64)], perm
