"""Meshes and a CPU oracle for quadric-error vertex placement in the clustering simplifier (mlsgpu_hip_mesh_simplify_quadric).

simplify_quadric() follows steps 3a-3h of the contract in include/mlsgpu_hip.h operation for operation in float64 / int64; the
cells, the clusters, the triangles, the numbering and the mean positions are simplify_cases.simplify's.  Nothing here is
product code.
"""
import numpy as np

import simplify_cases as sc

STAT_NAMES = sc.STAT_NAMES + ("solvedVertices", "flatVertices", "escapedVertices", "scaleExponent")
SUM_LIMIT = 2 ** 62


def simplify_quadric(vertices, triangles, origin, cell_size, details=None):
    """(vertices float32 [n, 3], triangles uint32 [m, 3], the ten statistics) or sc.Invalid.  With a dict as `details` the
    per-output-vertex state is left there: kind (0 single, 1 solved, 2 flat, 3 escaped), members, and A, b, mu, r, x, mean
    (cell coordinates centred on the cell) of the multi-member ones."""
    mean_v, out_t, stats = sc.simplify(vertices, triangles, origin, cell_size)
    stats = dict(stats, solvedVertices=0, flatVertices=0, escapedVertices=0, scaleExponent=0)
    p = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(p), len(tri)
    if V == 0 or T == 0:
        return mean_v, out_t, stats
    origin32, cell32 = np.asarray(origin, np.float32), np.float32(cell_size)
    origin64, cell64 = origin32.astype(np.float64), np.float64(cell32)
    c = sc.cells(p, origin32, cell32)
    ci = c.astype(np.int64)
    key = ci[:, 2] << 42 | ci[:, 1] << 21 | ci[:, 0]
    _, first_member, cluster_of, members = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    C = len(members)
    # 3b: cell coordinates and the centred offset of a vertex in its own cell
    g = (p.astype(np.float64) - origin64) / cell64
    w = (g - c.astype(np.float64)) - 0.5
    # 3c: face vectors
    g0, g1, g2 = g[tri[:, 0]], g[tri[:, 1]], g[tri[:, 2]]
    a, b = g1 - g0, g2 - g0
    n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                  a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    assert np.isfinite(n).all()
    # 3d: the scale
    M = float(np.abs(n).max())
    A = np.zeros((C, 6), np.int64)
    B = np.zeros((C, 3), np.int64)
    if M != 0.0:
        e = int(np.frexp(M)[1]) - 1
        E = 2 * e + 1
        shift = (60 - int(T).bit_length()) - E
        stats["scaleExponent"] = E
        # 3e: accumulation, once per distinct cluster of a triangle
        qa = np.rint(np.ldexp(np.stack([n[:, 0] * n[:, 0], n[:, 0] * n[:, 1], n[:, 0] * n[:, 2], n[:, 1] * n[:, 1],
                                        n[:, 1] * n[:, 2], n[:, 2] * n[:, 2]], axis=1), shift)).astype(np.int64)
        m = cluster_of[tri]
        adds = [np.ones(T, bool), m[:, 1] != m[:, 0], (m[:, 2] != m[:, 0]) & (m[:, 2] != m[:, 1])]
        count = np.zeros(C, np.int64)
        largest = int(np.abs(qa).max())
        for k in range(3):
            wk = w[tri[:, k]]
            d = -((n[:, 0] * wk[:, 0] + n[:, 1] * wk[:, 1]) + n[:, 2] * wk[:, 2])
            qb = np.rint(np.ldexp(d[:, None] * n, shift)).astype(np.int64)
            largest = max(largest, int(np.abs(qb).max()))
            np.add.at(A, m[adds[k], k], qa[adds[k]])
            np.add.at(B, m[adds[k], k], qb[adds[k]])
            np.add.at(count, m[adds[k], k], 1)
        # Python integers: no sum can have reached 2^62
        assert largest < 2 ** ((60 - int(T).bit_length()) + 2)
        assert largest * int(count.max()) < SUM_LIMIT
    # the mean, as simplify_cases.simplify takes it
    f = (p.astype(np.float64) - origin64) / cell64 - c.astype(np.float64)
    q = np.rint(f * sc.FIXED_ONE).astype(np.int64)
    S = np.zeros((C, 3), np.int64)
    np.add.at(S, cluster_of, q)
    mean = (S.astype(np.float64) / members.astype(np.float64)[:, None]) * (1.0 / sc.FIXED_ONE) - 0.5
    # 3f: the solve
    with np.errstate(all="ignore"):
        a00, a01, a02, a11, a12, a22 = (A[:, k].astype(np.float64) for k in range(6))
        tr = (a00 + a11) + a22
        mu = tr * 2.0 ** -10
        r = mu[:, None] * mean - B.astype(np.float64)
        d0 = a00 + mu
        l10 = a01 / d0
        l20 = a02 / d0
        d1 = (a11 + mu) - l10 * a01
        t = a12 - l20 * a01
        l21 = t / d1
        d2 = ((a22 + mu) - l20 * a02) - l21 * t
        y0 = r[:, 0]
        y1 = r[:, 1] - l10 * y0
        y2 = (r[:, 2] - l20 * y0) - l21 * y1
        z0, z1, z2 = y0 / d0, y1 / d1, y2 / d2
        x2 = z2
        x1 = z1 - l21 * x2
        x0 = (z0 - l10 * x1) - l20 * x2
        x = np.stack([x0, x1, x2], axis=1)
        inside = (np.isfinite(x) & (np.abs(x) <= 0.5)).all(axis=1)
    # 3a, 3g: 0 single, 1 solved, 2 flat, 3 escaped
    kind = np.where(members == 1, 0, np.where(tr == 0.0, 2, np.where(inside, 1, 3)))
    cluster_cell = c[first_member].astype(np.float64)
    with np.errstate(all="ignore"):
        solved_pos = (origin64 + ((cluster_cell + 0.5) + x) * cell64).astype(np.float32)
    # the clusters in use: those of the triangles that do not collapse, in key order
    m = cluster_of[tri]
    collapsed = (m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 2] == m[:, 0])
    used = np.zeros(C, bool)
    used[m[~collapsed].ravel()] = True
    assert used.sum() == len(mean_v)
    out_v = mean_v.copy()
    kind_out = kind[used]
    out_v[kind_out == 1] = solved_pos[used][kind_out == 1]
    stats["solvedVertices"] = int((kind_out == 1).sum())
    stats["flatVertices"] = int((kind_out == 2).sum())
    stats["escapedVertices"] = int((kind_out == 3).sum())
    assert stats["outVertices"] == int((kind_out == 0).sum()) + stats["solvedVertices"] + stats["flatVertices"] + stats["escapedVertices"]
    if details is not None:
        details.update(kind=kind_out, members=members[used], A=A[used], b=B[used], mu=mu[used], r=r[used], x=x[used],
                       mean=mean[used])
    return np.ascontiguousarray(out_v, np.float32), out_t, stats


def assert_same(got, want):
    """(vertices, triangles, the ten statistics) against the oracle's, bit for bit."""
    sc.assert_same(got, want)


# ---------------------------------------------------------------- meshes

def cube_mesh(n, L, jitter=0.0, seed=0):
    """The welded closed surface of the cube [0, L]^3 with n quads per edge, two triangles per quad, facing outwards.  Every
    vertex is moved by up to jitter * L / n (seeded) along the axes in which it is free: a face's vertex inside the face, an
    edge's along the edge, a corner not at all -- every vertex stays on the cube."""
    lattice = {}
    tri = []

    def vertex(i, j, k):
        return lattice.setdefault((i, j, k), len(lattice))

    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        q = [0, 0, 0]
                        q[axis], q[u], q[v] = side, i + di, j + dj
                        return vertex(*q)
                    quad = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]     # counter-clockwise seen from +axis
                    if side == 0:
                        quad.reverse()
                    tri.append([quad[0], quad[1], quad[2]])
                    tri.append([quad[0], quad[2], quad[3]])
    ijk = np.array(sorted(lattice, key=lattice.get), np.float64)
    free = (ijk != 0) & (ijk != n)
    move = np.random.default_rng(seed).uniform(-jitter, jitter, ijk.shape) if jitter else np.zeros_like(ijk)
    p = (ijk + move * free) * (L / n)
    return p.astype(np.float32), np.array(tri, np.uint32)


def cube_distance(points, L):
    """The distance of every point to the surface of the cube [0, L]^3."""
    q = np.asarray(points, np.float64)
    outside = np.maximum(np.maximum(-q, q - L), 0.0)
    out = np.sqrt((outside ** 2).sum(axis=1))
    inside = np.minimum(q, L - q).min(axis=1)
    return np.where((outside == 0).all(axis=1), inside, out)


def torus_distance(points, major, minor):
    """The distance of every point to the torus around the z axis through the origin."""
    q = np.asarray(points, np.float64)
    ring = np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2) - major
    return np.abs(np.sqrt(ring ** 2 + q[:, 2] ** 2) - minor)


def sheet(nx, ny, spacing, x0, height, slope):
    """nx * ny vertices of a grid in the plane z = height + slope * x, x from x0 and y from 0 in steps of `spacing`."""
    p, tri = sc.grid_mesh(nx, ny)
    p = p.astype(np.float64) * spacing
    p[:, 0] += x0
    p[:, 2] = height + slope * p[:, 0]
    return p, np.asarray(tri, np.int64)


def wedge_mesh():
    """Two sheets that are not joined, z = 0.1 and z = 0.1 + tan(20 deg) x, for x in [1.55, 4.3]: their line of intersection,
    x = 0, lies 1.5 to 4 cells of side 1 away from every vertex.  The cells x in [2, 3), z in [0, 1) hold vertices of both
    sheets: the minimiser of such a cluster's quadric lies near that line, outside the cell.  (origin, cell) to go with it."""
    slope = np.tan(np.radians(20.0))
    lower, lower_t = sheet(12, 13, 0.25, 1.55, 0.1, 0.0)
    upper, upper_t = sheet(12, 13, 0.25, 1.55, 0.1, slope)
    p = np.concatenate([lower, upper])
    tri = np.concatenate([lower_t, upper_t[:, ::-1] + len(lower)])
    return p.astype(np.float32), tri.astype(np.uint32), (0.0, -0.1, 0.0), 1.0


def line_mesh(count=40, offset=0.0):
    """Vertices on a straight line, 0.4 apart, and the triangles (i, i + 3, i + 6): every face vector is zero, and at a cell
    of 1 no triangle collapses."""
    p = np.zeros((count, 3), np.float64)
    p[:, 0] = 0.4 * np.arange(count)
    p[:, 1] = p[:, 2] = 0.3 + offset
    i = np.arange(count - 6)
    return p.astype(np.float32), np.stack([i, i + 3, i + 6], axis=1).astype(np.uint32)


def flat_and_grid_mesh():
    """line_mesh next to a jittered grid 20 cells above it: M != 0, and the line's clusters have tr == 0."""
    lp, lt = line_mesh()
    gp, gt = sc.grid_mesh(12, 12, jitter=0.3, seed=4)
    gp = gp * np.float32(0.5) + np.array([0.0, 0.0, 20.0], np.float32)
    return np.concatenate([lp, gp]).astype(np.float32), np.concatenate([lt, np.asarray(gt, np.uint32) + len(lp)]).astype(np.uint32)


def permuted_triangles(triangles, seed):
    t = np.asarray(triangles)
    return t[np.random.default_rng(seed).permutation(len(t))]


def renumbered(vertices, triangles, seed):
    """The same mesh with its vertices in another order."""
    order = np.random.default_rng(seed).permutation(len(vertices))     # new position -> old vertex
    new_of_old = np.empty(len(vertices), np.int64)
    new_of_old[order] = np.arange(len(vertices))
    return np.asarray(vertices)[order], new_of_old[np.asarray(triangles, np.int64)].astype(np.uint32)
