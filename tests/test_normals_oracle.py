"""The numpy oracle of the vertex-normal contract (normals_cases.normals) against what the contract promises: hand case,
an analytic surface, invariance under power-of-two scaling, triangle order and triple rotation, the counters, empty meshes."""
import numpy as np
import pytest

import normals_cases as nc


def bits(n):
    return np.ascontiguousarray(n, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def torus():
    p, tri = nc.torus_mesh(400, 60, 0.5, 0.125)
    return p, tri, nc.normals(p, tri)


def test_hand_case():
    p, tri = nc.grid_mesh(4, 4)
    n, st = nc.normals(p, tri)
    assert n.tolist() == [[0.0, 0.0, 1.0]] * 16
    assert st == dict(numVertices=16, numTriangles=18, outOfRangeTriangles=0, nonFiniteTriangles=0, zeroNormals=0, scaleExponent=0)


def test_torus_against_the_analytic_normal(torus):
    """The worst dot product is 0.9999998 (the mesh is a 400 x 60 polyhedron, not the torus): 0.99999 is a sanity margin."""
    p, tri, (n, st) = torus
    dot = (n.astype(np.float64) * nc.torus_normals(400, 60)).sum(axis=1)
    assert dot.min() >= 0.99999, dot.min()
    assert st["zeroNormals"] == 0 and st["outOfRangeTriangles"] == 0 and st["nonFiniteTriangles"] == 0


@pytest.mark.parametrize("shift", [-40, 40])
def test_power_of_two_scaling(torus, shift):
    """Scaling every coordinate by 2^shift is exact in float32 and multiplies every face vector by exactly 2^(2 shift): the
    same q, the same normals bit for bit, and scaleExponent moves by exactly twice the shift, -80 and +80.  (The issue that
    asked for this test quotes -71 and +89, "twice the shift, less nine", from a draft; its own step 3 -- 2^e <= M < 2^(e + 1)
    with M scaled by 2^(2 shift) -- allows nothing but 2 shift, and that is what is asserted.)"""
    p, tri, (n, st) = torus
    scaled, scaled_st = nc.normals(p * np.float32(2.0 ** shift), tri)
    np.testing.assert_array_equal(bits(scaled), bits(n))
    assert scaled_st["scaleExponent"] - st["scaleExponent"] == 2 * shift
    assert dict(scaled_st, scaleExponent=0) == dict(st, scaleExponent=0)


def test_triangle_order_and_rotation_leave_every_bit(torus):
    p, tri, want = torus
    rng = np.random.default_rng(7)
    nc.assert_same(nc.normals(p, tri[rng.permutation(len(tri))]), want)
    turn = rng.integers(0, 3, len(tri))
    rotated = np.stack([np.take_along_axis(tri, ((turn + k) % 3)[:, None], axis=1)[:, 0] for k in range(3)], axis=1)
    assert (turn != 0).sum() > 1000
    nc.assert_same(nc.normals(p, rotated), want)


def test_counters():
    """counter_mesh: two triangles out of range; vertex 40 at NaN and vertex 60 at infinity make the six triangles around
    each non-finite; vertex 99 is unused.  The vertex at 3e38 does NOT overflow (the products are doubles: 9e76 is finite):
    its triangles take part and set the scale, e = 128, against which the unit triangles quantise to nothing."""
    p, tri = nc.counter_mesh()
    n, st = nc.normals(p, tri)
    assert st["outOfRangeTriangles"] == 2 and st["nonFiniteTriangles"] == 12
    assert st["scaleExponent"] == 128 and (n[99] == 0).all() and st["zeroNormals"] >= 1
    around = np.unique(tri[(tri == 16).any(axis=1) & (tri < len(p)).all(axis=1)])
    assert (np.abs(n[around]).sum(axis=1) > 0).all()
    # without the far vertex the scale is the grid's and every used vertex away from the bad ones has a normal
    p[16, 2] = 0.0
    n, st = nc.normals(p, tri)
    assert (st["outOfRangeTriangles"], st["nonFiniteTriangles"]) == (2, 12) and -2 <= st["scaleExponent"] <= 2
    assert (n[99] == 0).all() and (n[40] == 0).all() and (n[60] == 0).all() and st["zeroNormals"] == 3
    assert np.isfinite(n).all()
    length = np.sqrt((n.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(length[np.abs(n).sum(axis=1) > 0] - 1).max() < 1e-6


def test_empty_meshes():
    p, tri = nc.grid_mesh(4, 4)
    n, st = nc.normals(p[:0], tri[:0])
    assert n.shape == (0, 3) and st == dict.fromkeys(nc.STAT_NAMES, 0)
    n, st = nc.normals(p, tri[:0])
    assert not n.any() and st == dict(dict.fromkeys(nc.STAT_NAMES, 0), numVertices=16, zeroNormals=16)
    n, st = nc.normals(p[:0], tri)                 # every index is out of range
    assert n.shape == (0, 3) and st == dict(dict.fromkeys(nc.STAT_NAMES, 0), numTriangles=18, outOfRangeTriangles=18)
