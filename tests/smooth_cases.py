"""A CPU oracle for the Taubin smoothing (mlsgpu_hip_mesh_smooth), and the meshes its tests share.

smooth() follows the contract in include/mlsgpu_hip.h step by step: np.unique on the undirected edges for the counts and the
neighbour sets, np.ldexp / np.rint for the fixed-point values, np.add.at on int64 for the sums (integers: the order does not
matter, and int64 arrays wrap).  Nothing here is product code.
"""
import numpy as np

from simplify_cases import grid_mesh, torus_mesh  # noqa: F401  (the tests take their meshes from here)

FIXED, CURVE = 0, 1
STAT_NAMES = ("numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "numEdges", "boundaryEdges",
              "boundaryVertices", "isolatedVertices", "passes", "scaleExponent", "maxMove", "maxCoordinate")


class Invalid(Exception):
    """What the device reports as MLSGPU_ERR_INVALID."""


def adjacency(num_vertices, triangles, boundary=FIXED):
    """Steps 1-3: (src, dst) of every (v, n) with n in N(v), k per vertex, the boundary mask, the counts as a dict."""
    V = num_vertices
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    bad = ((tri >= V) | (tri < 0)).any(axis=1)
    degenerate = ~bad & ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0]))
    part = tri[~bad & ~degenerate]
    a, b = part.ravel(), part[:, [1, 2, 0]].ravel()             # the three sides of every participating triangle
    lo, hi = np.minimum(a, b).astype(np.uint64), np.maximum(a, b).astype(np.uint64)
    code, uses = np.unique(lo << np.uint64(32) | hi, return_counts=True)
    lo, hi = (code >> np.uint64(32)).astype(np.int64), (code & np.uint64(0xFFFFFFFF)).astype(np.int64)
    single = uses == 1                                          # a -> b and b -> a counted together
    on_boundary = np.zeros(V, bool)
    on_boundary[lo[single]] = True
    on_boundary[hi[single]] = True
    used = np.zeros(V, bool)
    used[lo] = True
    used[hi] = True
    src, dst, edge_single = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([single, single])
    keep = ~on_boundary[src] | (edge_single if boundary == CURVE else False)
    src, dst = src[keep], dst[keep]
    counts = dict(outOfRangeTriangles=int(bad.sum()), degenerateTriangles=int(degenerate.sum()), numEdges=len(code),
                  boundaryEdges=int(single.sum()), boundaryVertices=int(on_boundary.sum()), isolatedVertices=int(V - used.sum()))
    return src, dst, np.bincount(src, minlength=V).astype(np.int64), on_boundary, counts


def smooth(vertices, triangles, iterations, lam, mu, boundary=FIXED):
    """(vertices float32 [V, 3], statistics dict) or Invalid."""
    p0 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    lam, mu = np.float32(lam), np.float32(mu)
    if not (np.isfinite(lam) and np.isfinite(mu) and 0 < lam <= 1 and -1 <= mu <= 0) or boundary not in (FIXED, CURVE):
        raise Invalid("parameters")
    if not np.isfinite(p0).all():
        raise Invalid("vertex")
    V = len(p0)
    src, dst, k, _, counts = adjacency(V, tri, boundary)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats.update(counts, numVertices=V, numTriangles=len(tri), passes=int(iterations) * (2 if mu != 0 else 1), maxMove=0.0, maxCoordinate=0.0)
    M = float(np.abs(p0).max()) if V else 0.0
    stats["maxCoordinate"] = M
    if M == 0:                                                  # step 4: the output is the input
        return p0.copy(), stats
    e = int(np.frexp(M)[1]) - 1                                 # 2^e <= M < 2^(e + 1)
    stats["scaleExponent"] = e
    moving = k > 0
    kf = k[moving].astype(np.float64)[:, None]
    p = p0.copy()
    for f in [lam, mu][:2 if mu != 0 else 1] * int(iterations):
        Q = np.rint(np.ldexp(p.astype(np.float64), 30 - e)).astype(np.int64)           # step 5
        S = np.zeros((V, 3), np.int64)
        np.add.at(S, src, Q[dst])
        D = S[moving] - k[moving][:, None] * Q[moving]
        d = np.ldexp(D.astype(np.float64) / kf, e - 30)
        out = p.copy()
        with np.errstate(over="ignore"):
            out[moving] = (p[moving].astype(np.float64) + np.float64(f) * d).astype(np.float32)
        p = out
        stats["maxCoordinate"] = max(stats["maxCoordinate"], float(np.abs(p).max()))
        if not np.isfinite(p).all() or stats["maxCoordinate"] > 2.0 ** (e + 21):        # step 7, before a value leaves int64
            raise Invalid("diverged: %g" % stats["maxCoordinate"])
    stats["maxMove"] = float(np.abs(p.astype(np.float64) - p0.astype(np.float64)).max())
    return p, stats


def assert_same(got, want):
    """(vertices, stats) against the oracle's: the positions as uint32 views, every statistic exactly."""
    gv, gs = got
    wv, ws = want
    assert gs == ws, (gs, ws)
    gv = np.ascontiguousarray(gv, np.float32).reshape(-1, 3)
    assert gv.shape == wv.shape
    np.testing.assert_array_equal(gv.view(np.uint32), wv.view(np.uint32))


# ---------------------------------------------------------------- meshes

def octahedron():
    """+-1 on the axes, eight outward triangles: closed, every vertex of valence 4."""
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    tri = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)
    return p, tri


def noisy_torus(n, m, sigma, seed, major=0.5, minor=0.125, centre=(0.0, 0.0, 0.0)):
    """torus_mesh(n, m, major, minor) with normal noise of standard deviation sigma on every coordinate (seeded)."""
    p, tri = torus_mesh(n, m, major, minor, centre)
    return (p.astype(np.float64) + np.random.default_rng(seed).normal(0, sigma, p.shape)).astype(np.float32), tri


def torus_distance(p, major=0.5, minor=0.125):
    """Signed distance of every row of p to the torus around the origin: positive outside the tube."""
    p = np.asarray(p, np.float64)
    return np.hypot(np.hypot(p[:, 0], p[:, 1]) - major, p[:, 2]) - minor


def split_torus(p, tri, n, m, at):
    """The triangles of torus_mesh(n, m, ...) whose ring i is below `at` and the others, as two meshes with their own vertex
    numbering: [(vertices, triangles, the input's index of every vertex)] * 2.  Triangles i * m + j and n * m + i * m + j are the
    quad between the rings i and i + 1."""
    ring = np.arange(len(tri)) % (n * m) // m
    halves = []
    for mask in (ring < at, ring >= at):
        t = tri[mask]
        ids, local = np.unique(t, return_inverse=True)
        halves.append((p[ids], local.reshape(-1, 3), ids))
    return halves


def renumbered(p, tri, seed):
    """The same mesh with its vertices in another order: (vertices, triangles, perm) with new vertex perm[v] = old vertex v."""
    perm = np.random.default_rng(seed).permutation(len(p))
    q = np.empty_like(p)
    q[perm] = p
    return q, perm[np.asarray(tri, np.int64)], perm
