"""Meshes with positions and a CPU oracle for the vertex-clustering simplifier (mlsgpu_hip_mesh_simplify).

simplify() follows the contract in include/mlsgpu_hip.h step by step: float32 arrays for the cells, float64 / int64 for the
positions, lexsort / unique for the triangles.  Nothing here is product code.
"""
import numpy as np

import topology_cases as tc

CELL_LIMIT = 2 ** 21
FIXED_ONE = float(2 ** 30)
STAT_NAMES = ("inVertices", "inTriangles", "outVertices", "outTriangles", "collapsedTriangles", "duplicateTriangles")


class Invalid(Exception):
    """What the device reports as MLSGPU_ERR_INVALID."""


def cells(vertices, origin, cell_size):
    """Step 1: the float32 cell per axis of every vertex, as float32 (not yet range-checked)."""
    p = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    origin = np.asarray(origin, np.float32)
    with np.errstate(all="ignore"):
        return np.floor((p - origin) / np.float32(cell_size))


def simplify(vertices, triangles, origin, cell_size):
    """(vertices float32 [n, 3], triangles uint32 [m, 3], statistics dict) or Invalid."""
    p = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    origin = np.asarray(origin, np.float32)
    cell_size = np.float32(cell_size)
    V, T = len(p), len(tri)
    if not (np.isfinite(cell_size) and cell_size > 0) or not np.isfinite(origin).all():
        raise Invalid("frame")
    c = cells(p, origin, cell_size)
    if not np.isfinite(p).all() or not ((c >= 0) & (c < CELL_LIMIT)).all():
        raise Invalid("vertex")
    if (tri >= V).any() or (tri < 0).any():
        raise Invalid("index")
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats["inVertices"], stats["inTriangles"] = V, T
    empty = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), stats
    if V == 0 or T == 0:
        return empty
    # steps 1-2: keys and clusters in ascending key order
    ci = c.astype(np.int64)
    key = ci[:, 2] << 42 | ci[:, 1] << 21 | ci[:, 0]
    cluster_key, first_member, cluster_of, members = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    C = len(cluster_key)
    # step 3: positions
    d = p.astype(np.float64) - origin.astype(np.float64)
    f = d / np.float64(cell_size) - c.astype(np.float64)
    q = np.rint(f * FIXED_ONE).astype(np.int64)
    S = np.zeros((C, 3), np.int64)
    np.add.at(S, cluster_of, q)
    mean = (S.astype(np.float64) / members.astype(np.float64)[:, None]) * (1.0 / FIXED_ONE)
    cluster_cell = c[first_member].astype(np.float64)
    pos = (origin.astype(np.float64) + (cluster_cell + mean) * np.float64(cell_size)).astype(np.float32)
    single = members == 1
    pos[single] = p[first_member[single]]
    # step 4: triangles
    m = cluster_of[tri]
    collapsed = (m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 2] == m[:, 0])
    stats["collapsedTriangles"] = int(collapsed.sum())
    m = m[~collapsed]
    shift = np.argmin(m, axis=1)
    m = np.stack([np.take_along_axis(m, ((shift + k) % 3)[:, None], axis=1)[:, 0] for k in range(3)], axis=1)
    m = m[np.lexsort((m[:, 2], m[:, 1], m[:, 0]))]
    kept = np.unique(m, axis=0) if len(m) else m            # rows in lexicographic order
    stats["duplicateTriangles"] = len(m) - len(kept)
    # step 5: the clusters in use, densely renumbered in key order
    used = np.zeros(C, bool)
    used[kept.ravel()] = True
    new_index = np.cumsum(used) - 1
    out_v = pos[used]
    out_t = new_index[kept].astype(np.uint32).reshape(-1, 3)
    stats["outVertices"], stats["outTriangles"] = len(out_v), len(out_t)
    assert T == stats["outTriangles"] + stats["collapsedTriangles"] + stats["duplicateTriangles"]
    return np.ascontiguousarray(out_v, np.float32), out_t, stats


def canonical(triangles):
    """Index triples rotated so that the smallest index comes first, as a sorted list of tuples."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    shift = np.argmin(t, axis=1) if len(t) else np.zeros(0, np.int64)
    rows = np.stack([np.take_along_axis(t, ((shift + k) % 3)[:, None], axis=1)[:, 0] for k in range(3)], axis=1) if len(t) else t
    return sorted(map(tuple, rows.tolist()))


def assert_same(got, want):
    """(vertices, triangles, stats) against the oracle's, bit for bit."""
    gv, gt, gs = got
    wv, wt, ws = want
    assert gs == ws, (gs, ws)
    assert gv.shape == wv.shape and gt.shape == wt.shape
    np.testing.assert_array_equal(np.ascontiguousarray(gv, np.float32).view(np.uint32), wv.view(np.uint32))
    np.testing.assert_array_equal(np.asarray(gt, np.uint32), wt)


# ---------------------------------------------------------------- meshes

def grid_mesh(n, m, jitter=0.0, seed=0):
    """tc.grid(n, m) with vertex i * m + j at (i, j, 0), each coordinate moved by up to `jitter` (seeded)."""
    V, tri = tc.grid(n, m)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), np.zeros(V)], axis=1).astype(np.float64)
    if jitter:
        p += np.random.default_rng(seed).uniform(-jitter, jitter, p.shape)
    return p.astype(np.float32), tri


def torus_mesh(n, m, major, minor, centre=(0.0, 0.0, 0.0), windings=1):
    """tc.torus(n, m): vertex i * m + j at angle i around the axis (radius `major`) and j around the tube (`minor`).  With
    `windings` = 2 (and n odd) the tube goes around the axis twice before it closes, through the same space: two layers with
    the SAME orientation -- what makes duplicate triangles.  (The two sides of one thin tube face opposite ways: they give
    (a, b, c) and (a, c, b), which both stay.)"""
    V, tri = tc.torus(n, m)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a, b = 2 * np.pi * windings * i.ravel() / n, 2 * np.pi * j.ravel() / m
    r = major + minor * np.cos(b)
    p = np.stack([r * np.cos(a), r * np.sin(a), minor * np.sin(b)], axis=1) + np.asarray(centre, np.float64)
    return p.astype(np.float32), tri
