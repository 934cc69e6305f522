"""A CPU oracle for the area-weighted vertex normals (mlsgpu_hip_mesh_normals), and the meshes its tests share.

normals() follows the contract in include/mlsgpu_hip.h step by step: float64 arrays for the face vectors, np.ldexp / np.rint
for the fixed-point values, np.add.at on int64 for the sums (integers: the order does not matter).  Nothing here is product
code.
"""
import numpy as np

from simplify_cases import grid_mesh, torus_mesh  # noqa: F401  (the tests take their meshes from here)

STAT_NAMES = ("numVertices", "numTriangles", "outOfRangeTriangles", "nonFiniteTriangles", "zeroNormals", "scaleExponent")


def face_vectors(vertices, triangles):
    """Steps 1 and 2: (c float64 [T, 3] with zero rows for the triangles that take no part, out-of-range mask, non-finite mask)."""
    p = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    V = len(p)
    bad = ((tri >= V) | (tri < 0)).any(axis=1)
    safe = np.where(bad[:, None], 0, tri) if V else np.zeros_like(tri)
    c = np.zeros((len(tri), 3), np.float64)
    if V:
        with np.errstate(all="ignore"):
            a = p[safe[:, 1]] - p[safe[:, 0]]
            b = p[safe[:, 2]] - p[safe[:, 0]]
            c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                          a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                          a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    non_finite = ~bad & ~np.isfinite(c).all(axis=1)
    c[bad | non_finite] = 0.0
    return c, bad, non_finite


def normals(vertices, triangles):
    """(normals float32 [V, 3], statistics dict)."""
    V = len(np.asarray(vertices).reshape(-1, 3))
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    c, bad, non_finite = face_vectors(vertices, tri)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats.update(numVertices=V, numTriangles=len(tri), outOfRangeTriangles=int(bad.sum()), nonFiniteTriangles=int(non_finite.sum()))
    S = np.zeros((V, 3), np.int64)
    M = np.abs(c).max() if c.size else 0.0
    if M > 0:
        e = int(np.frexp(M)[1]) - 1                 # step 3: 2^e <= M < 2^(e + 1)
        q = np.rint(np.ldexp(c, 30 - e)).astype(np.int64)
        assert np.abs(q).max() <= 2 ** 31
        stats["scaleExponent"] = e
        part = ~(bad | non_finite)
        for corner in range(3):                     # step 4
            np.add.at(S, tri[part, corner], q[part])
    x = S.astype(np.float64)                        # step 5
    l = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    zero = l == 0
    with np.errstate(all="ignore"):
        n = (x / l[:, None]).astype(np.float32)
    n[zero] = 0.0
    stats["zeroNormals"] = int(zero.sum())
    return n, stats


def assert_same(got, want):
    """(normals, stats) against the oracle's: the normals as uint32 views, all statistics."""
    gn, gs = got
    wn, ws = want
    assert gs == ws, (gs, ws)
    gn = np.ascontiguousarray(gn, np.float32).reshape(-1, 3)
    assert gn.shape == wn.shape
    np.testing.assert_array_equal(gn.view(np.uint32), wn.view(np.uint32))


# ---------------------------------------------------------------- meshes

def fan_mesh(n, seed=0):
    """n triangles (0, i, i + 1) around hub vertex 0, the rim a closed, slightly irregular ring below the hub."""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n) / n
    r = 1.0 + 0.2 * rng.uniform(-1, 1, n)
    rim = np.stack([r * np.cos(a), r * np.sin(a), 0.1 * rng.uniform(-1, 1, n)], axis=1)
    p = np.concatenate([[[0.0, 0.0, 0.5]], rim]).astype(np.float32)
    i = np.arange(n)
    tri = np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], axis=1)
    return p, tri


def counter_mesh():
    """A 9 x 11 grid with what the counters count: two triangles with an index >= V (one of them 0xFFFFFFFF), a vertex at
    NaN and one at infinity (their triangles' face vectors are not finite), a vertex at 3e38 (finite in double: it takes part
    and sets the scale, so the unit triangles quantise to nothing) and an unused vertex appended at the end."""
    p, tri = grid_mesh(9, 11, jitter=0.2, seed=3)
    p = np.concatenate([p, [[4.0, 4.0, 1.0]]]).astype(np.float32)     # vertex 99: unused
    tri = tri.copy()
    tri[5, 2] = len(p)
    tri[77, 0] = 0xFFFFFFFF
    p[40, 1] = np.nan
    p[60, 0] = np.inf
    p[16, 2] = 3e38
    return p, tri


def torus_normals(n, m):
    """The analytic unit normal of torus_mesh(n, m, ...) at every vertex: outwards from the tube's centre line."""
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    a, b = 2 * np.pi * i.ravel() / n, 2 * np.pi * j.ravel() / m
    return np.stack([np.cos(b) * np.cos(a), np.cos(b) * np.sin(a), np.sin(b)], axis=1)
