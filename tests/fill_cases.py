"""A CPU oracle for the hole filling (mlsgpu_hip_mesh_fill_holes), and the meshes its tests share.

fill() follows the contract in include/mlsgpu_hip.h step by step: np.unique on the directed sides for the boundary, hooking
and pointer jumping over the boundary vertices for the components (no Python loop per vertex), np.ldexp / np.rint for the
fixed-point values, np.add.at on int64 for the sums.  Nothing here is product code.
"""
import numpy as np

from simplify_cases import grid_mesh, torus_mesh  # noqa: F401  (the tests take their meshes from here)
from smooth_cases import octahedron, renumbered  # noqa: F401

MAX_EDGES_LIMIT = 2 ** 20
STAT_NAMES = ("numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "boundaryEdges", "irregularEdges",
              "loops", "filledLoops", "longLoops", "pinnedLoops", "filledEdges", "longestLoop", "outVertices", "outTriangles",
              "scaleExponent")


class Invalid(Exception):
    """What the device reports as MLSGPU_ERR_INVALID."""


def boundary_sides(num_vertices, triangles):
    """Steps 1 and 2: (from, to) of every boundary side in ascending (from, to) order, and the two counts of step 1."""
    V = int(num_vertices)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    bad = ((tri >= V) | (tri < 0)).any(axis=1)
    degenerate = ~bad & ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0]))
    part = tri[~bad & ~degenerate]
    a, b = part.ravel().astype(np.uint64), part[:, [1, 2, 0]].ravel().astype(np.uint64)
    code, uses = np.unique(a << np.uint64(32) | b, return_counts=True)
    ua, ub = code >> np.uint64(32), code & np.uint64(0xFFFFFFFF)
    opposite = np.isin(ub << np.uint64(32) | ua, code)
    side = (uses == 1) & ~opposite
    return ua[side].astype(np.int64), ub[side].astype(np.int64), int(bad.sum()), int(degenerate.sum())


def components(n, a, b):
    """The smallest member of the connected component of each of 0 .. n - 1 under the edges (a[k], b[k]): roots hook under
    smaller roots, then every pointer jumps until it points at a root; the components at least halve per round."""
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        live = lo != hi
        if not live.any():
            return parent
        np.minimum.at(parent, hi[live], lo[live])
        while True:
            jumped = parent[parent]
            if np.array_equal(jumped, parent):
                break
            parent = jumped


def fill(vertices, triangles, max_edges, pinned=None):
    """(vertices float32 [V', 3], triangles uint32 [T', 3], statistics dict) or Invalid."""
    p = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    if not 3 <= int(max_edges) <= MAX_EDGES_LIMIT:
        raise Invalid("max_edges")
    if not np.isfinite(p).all():
        raise Invalid("vertex")
    V, T = len(p), len(tri)
    fa, fb, bad, degenerate = boundary_sides(V, tri)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats.update(numVertices=V, numTriangles=T, outOfRangeTriangles=bad, degenerateTriangles=degenerate, boundaryEdges=len(fa))
    M = float(np.abs(p).max()) if V else 0.0
    e = int(np.frexp(M)[1]) - 1 if M > 0 else 0                 # step 6: 2^e <= M < 2^(e + 1)
    stats["scaleExponent"] = e

    # steps 3 and 4, over the boundary vertices in ascending order (so the smallest local number is the smallest vertex)
    ids = np.unique(np.concatenate([fa, fb]))
    la, lb = np.searchsorted(ids, fa), np.searchsorted(ids, fb)
    n = len(ids)
    out_count, in_count = np.bincount(la, minlength=n), np.bincount(lb, minlength=n)
    regular = (out_count == 1) & (in_count == 1)
    root = components(n, la, lb)
    length = np.bincount(root, minlength=n)                     # vertices per component, at its root
    irregular = np.zeros(n, bool)
    irregular[root[~regular]] = True
    pin = np.zeros(n, bool)
    if pinned is not None:
        mask = np.asarray(pinned).reshape(-1) != 0
        assert len(mask) == V
        pin[root[mask[ids]]] = True
    is_root = (root == np.arange(n)) & (length > 0)
    loop = is_root & ~irregular
    assert (length[loop] >= 3).all()
    stats["irregularEdges"] = int(out_count[irregular[root]].sum())
    stats["loops"] = int(loop.sum())
    stats["longestLoop"] = int(length[loop].max()) if loop.any() else 0
    long_ = loop & (length > int(max_edges))                    # step 5: long before pinned
    pinned_ = loop & ~long_ & pin
    filled = loop & ~long_ & ~pinned_
    stats.update(longLoops=int(long_.sum()), pinnedLoops=int(pinned_.sum()), filledLoops=int(filled.sum()),
                 filledEdges=int(length[filled].sum()))

    # steps 7 and 8
    number = np.cumsum(filled) - 1                              # at a filled root: its j
    member = filled[root]                                       # the vertices of the filled loops, every one regular
    Q = np.rint(np.ldexp(p[ids[member]].astype(np.float64), 30 - e)).astype(np.int64)
    S = np.zeros((n, 3), np.int64)
    np.add.at(S, root[member], Q)
    new_vertices = np.ldexp(S[filled].astype(np.float64) / length[filled].astype(np.float64)[:, None], e - 30).astype(np.float32)

    # steps 9 and 10: the side that leaves a, in ascending order of a
    nxt = np.zeros(n, np.int64)
    nxt[la] = lb                                                # one side per regular vertex
    a = np.flatnonzero(member)
    new_triangles = np.stack([ids[nxt[a]], ids[a], V + number[root[a]]], axis=1) if len(a) else np.zeros((0, 3), np.int64)
    out_v = np.concatenate([p, new_vertices.reshape(-1, 3)])
    out_t = np.concatenate([tri, new_triangles]).astype(np.uint32)
    stats.update(outVertices=len(out_v), outTriangles=len(out_t))
    assert stats["outVertices"] == V + stats["filledLoops"] and stats["outTriangles"] == T + stats["filledEdges"]
    return out_v, out_t, stats


def assert_same(got, want):
    """(vertices, triangles, stats) against the oracle's: the positions as uint32 views, triangles and every statistic exactly."""
    gv, gt, gs = got
    wv, wt, ws = want
    assert gs == ws, (gs, ws)
    gv = np.ascontiguousarray(gv, np.float32).reshape(-1, 3)
    assert gv.shape == wv.shape
    np.testing.assert_array_equal(gv.view(np.uint32), wv.view(np.uint32))
    np.testing.assert_array_equal(np.asarray(gt, np.uint32).reshape(-1, 3), wt)


def soup(vertices, triangles):
    """The mesh as a sorted list of triangles over position bytes, each rotated so that its smallest corner comes first: what
    renumbering the vertices leaves alone."""
    rows = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).view(np.uint32)
    out = []
    for t in np.asarray(triangles, np.int64).reshape(-1, 3):
        corners = [tuple(int(x) for x in rows[i]) for i in t]
        k = corners.index(min(corners))
        out.append(tuple(corners[k:] + corners[:k]))
    return sorted(out)


# ---------------------------------------------------------------- meshes

def compacted(p, tri):
    """The mesh without the vertices that no triangle uses, the others in their order."""
    ids, local = np.unique(np.asarray(tri, np.int64), return_inverse=True)
    return p[ids], local.reshape(-1, 3).astype(np.int64)


def punched(n, m, holes, jitter=0.0, seed=0, compact=False):
    """grid_mesh(n, m, jitter, seed) without the quads of each (i0, j0, h, w) in holes: quads i0 .. i0 + h - 1 by
    j0 .. j0 + w - 1, a hole of 2 (h + w) sides.  The (h - 1) (w - 1) vertices inside a hole stay, unused, unless compact."""
    p, tri = grid_mesh(n, m, jitter, seed)
    keep = np.ones(len(tri), bool)
    for i0, j0, h, w in holes:
        i, j = np.meshgrid(np.arange(i0, i0 + h), np.arange(j0, j0 + w), indexing="ij")
        quad = (i * (m - 1) + j).ravel()
        keep[2 * quad] = False
        keep[2 * quad + 1] = False
    tri = tri[keep]
    return compacted(p, tri) if compact else (p, tri)


def punched_torus(n, m, holes, major=0.5, minor=0.125):
    """torus_mesh(n, m, major, minor) without the quads of each (i0, j0, h, w) in holes (no wrap-around), compacted."""
    p, tri = torus_mesh(n, m, major, minor)
    keep = np.ones(len(tri), bool)
    for i0, j0, h, w in holes:
        i, j = np.meshgrid(np.arange(i0, i0 + h), np.arange(j0, j0 + w), indexing="ij")
        quad = (i * m + j).ravel()
        keep[quad] = False
        keep[n * m + quad] = False
    return compacted(p, tri[keep])


def figure_eight(n=6, m=6, at=(2, 2), jitter=0.0, seed=0):
    """A grid with two unit holes that touch at a corner: the corner has two boundary sides out and two in, so it is
    irregular, and the 8 sides of the two holes are one component that is never filled."""
    return punched(n, m, [(at[0], at[1], 1, 1), (at[0] + 1, at[1] + 1, 1, 1)], jitter, seed)
