"""The contract of the Taubin smoothing (include/mlsgpu_hip.h) on the CPU oracle of smooth_cases.py: the hand cases, the
invariances the contract promises, what the filter does to a noisy torus, the seam between two halves, divergence."""
import numpy as np
import pytest

import smooth_cases as sc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- hand cases

def test_octahedron():
    p, tri = sc.octahedron()
    out, st = sc.smooth(p, tri, 1, 0.5, -0.5)
    assert out.tolist() == (p * 0.75).tolist() and (np.abs(out).sum(axis=1) == 0.75).all()
    assert st == dict(numVertices=6, numTriangles=8, outOfRangeTriangles=0, degenerateTriangles=0, numEdges=12, boundaryEdges=0,
                      boundaryVertices=0, isolatedVertices=0, passes=2, scaleExponent=0, maxMove=0.25, maxCoordinate=1.0)
    # the lambda pass alone: every vertex to the mean of its ring, the centre of the octahedron's equator
    assert sc.smooth(p, tri, 1, 1.0, 0.0)[0].tolist() == np.zeros((6, 3)).tolist()


def test_flat_grid():
    p, tri = sc.grid_mesh(4, 4)
    out, st = sc.smooth(p, tri, 3, 0.5, -0.53)
    assert (st["numEdges"], st["boundaryEdges"], st["boundaryVertices"], st["isolatedVertices"]) == (33, 12, 12, 0)
    assert (st["passes"], st["scaleExponent"], st["maxMove"], st["maxCoordinate"]) == (6, 1, 0.0, 3.0)
    np.testing.assert_array_equal(bits(out), bits(p))           # FIXED: the rim stays, the interior balances
    out, st = sc.smooth(p, tri, 3, 0.5, -0.53, sc.CURVE)
    corners = [0, 3, 12, 15]
    assert (out[corners, :2] != p[corners, :2]).all() and st["maxMove"] > 0.1
    inner = [5, 6, 9, 10]
    assert (out[:, 2] == 0).all() and st["boundaryVertices"] == 12
    # an interior vertex moves only because the rim under it has moved
    assert not np.array_equal(bits(out[inner]), bits(p[inner]))


def test_counts_of_a_mesh_with_defects():
    p, tri = sc.grid_mesh(4, 4)
    p = np.concatenate([p, [[9.0, 9.0, 9.0]]]).astype(np.float32)       # vertex 16: unused
    tri = np.concatenate([tri, [[0, 1, 17], [5, 5, 6], [0xFFFFFFFF, 1, 2], [3, 2, 3]]])
    _, st = sc.smooth(p, tri, 1, 0.5, -0.53)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["isolatedVertices"], st["numEdges"]) == (2, 2, 1, 33)
    # a side used twice in the same direction is no boundary: every triangle twice leaves nothing on the boundary
    p, tri = sc.grid_mesh(4, 4)
    _, st = sc.smooth(p, np.concatenate([tri, tri]), 1, 0.5, -0.53)
    assert (st["numEdges"], st["boundaryEdges"], st["boundaryVertices"]) == (33, 0, 0)


def test_classification_differs_from_the_topology_report():
    import topology_cases as tc
    p, tri = tc.classification_trap()
    tc.assert_trap_report(tc.count_all(len(p), tri))                # there: one out of range, two degenerate
    for mode in (sc.FIXED, sc.CURVE):
        out, st = sc.smooth(p, tri, 2, 0.5, -0.53, mode)
        assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 1)     # here: (1, 1, 7) is out of range
        assert (st["numEdges"], st["boundaryEdges"], st["boundaryVertices"], st["isolatedVertices"]) == (5, 4, 4, 0)
        assert out.tobytes() == sc.smooth(p, tri[:2], 2, 0.5, -0.53, mode)[0].tobytes()     # the bad ones take no part


# ---------------------------------------------------------------- invariances

@pytest.fixture(scope="module")
def jittered():
    p, tri = sc.grid_mesh(9, 11, jitter=0.2, seed=3)
    return p, tri, {mode: sc.smooth(p, tri, 3, 0.5, -0.53, mode) for mode in (sc.FIXED, sc.CURVE)}


@pytest.mark.parametrize("mode", [sc.FIXED, sc.CURVE])
def test_triangle_order_does_not_matter(jittered, mode):
    p, tri, want = jittered
    shuffled = tri[np.random.default_rng(5).permutation(len(tri))]
    sc.assert_same(sc.smooth(p, shuffled, 3, 0.5, -0.53, mode), want[mode])
    rotated = np.roll(tri, 1, axis=1)                           # the same triangles, another first corner
    sc.assert_same(sc.smooth(p, rotated, 3, 0.5, -0.53, mode), want[mode])


@pytest.mark.parametrize("mode", [sc.FIXED, sc.CURVE])
def test_renumbering_permutes_the_output(jittered, mode):
    p, tri, want = jittered
    q, qtri, perm = sc.renumbered(p, tri, 6)
    out, st = sc.smooth(q, qtri, 3, 0.5, -0.53, mode)
    assert st == want[mode][1]
    np.testing.assert_array_equal(bits(out[perm]), bits(want[mode][0]))


@pytest.mark.parametrize("mode", [sc.FIXED, sc.CURVE])
def test_power_of_two_scaling_is_exact(jittered, mode):
    p, tri, want = jittered
    s = np.float32(2.0 ** -7)
    out, st = sc.smooth(p * s, tri, 3, 0.5, -0.53, mode)
    np.testing.assert_array_equal(bits(out), bits(want[mode][0] * s))
    assert (want[mode][1]["scaleExponent"], st["scaleExponent"]) == (3, -4)
    assert st["maxMove"] == want[mode][1]["maxMove"] * 2.0 ** -7 and st["maxCoordinate"] == want[mode][1]["maxCoordinate"] * 2.0 ** -7


# ---------------------------------------------------------------- what the filter does

@pytest.fixture(scope="module")
def torus():
    return sc.noisy_torus(200, 40, 0.004, 7)


def rms(d):
    return float(np.sqrt((d * d).mean()))


def test_taubin_denoises_without_shrinking(torus):
    """The figures of the contract's prototype: input rms 0.003974; ten iterations (0.5, -0.53) rms 0.001505, mean +0.000216;
    ten plain Laplacian iterations (0.5, 0) mean -0.005209."""
    p, tri = torus
    before = rms(sc.torus_distance(p))
    assert abs(before - 0.003974) < 1e-6
    taubin = sc.torus_distance(sc.smooth(p, tri, 10, 0.5, -0.53)[0])
    laplace = sc.torus_distance(sc.smooth(p, tri, 10, 0.5, 0.0)[0])
    assert rms(taubin) < 0.5 * before and abs(taubin.mean()) < 0.001
    assert laplace.mean() < -0.004
    assert abs(rms(taubin) - 0.001505) < 1e-6 and abs(taubin.mean() - 0.000216) < 1e-6 and abs(laplace.mean() + 0.005209) < 1e-6


def test_seam_between_two_halves_stays_closed(torus):
    p, tri = torus
    halves = sc.split_torus(p, tri, 200, 40, 100)
    shared = np.intersect1d(halves[0][2], halves[1][2])
    assert len(shared) == 80
    for v, t, ids in halves:
        out, st = sc.smooth(v, t, 10, 0.5, -0.53, sc.FIXED)
        assert st["boundaryVertices"] == 80 and st["isolatedVertices"] == 0 and st["maxMove"] > 0.001
        local = np.searchsorted(ids, shared)
        np.testing.assert_array_equal(bits(out[local]), bits(p[shared]))
        # under CURVE the seam's vertices slide along their ring
        assert not np.array_equal(bits(sc.smooth(v, t, 10, 0.5, -0.53, sc.CURVE)[0][local]), bits(p[shared]))


# ---------------------------------------------------------------- divergence, empty meshes, parameters

def test_divergence_is_an_error():
    p, tri = sc.noisy_torus(40, 12, 0.01, 1)
    out, st = sc.smooth(p, tri, 40, 0.3, -1.0)
    assert 2.0e4 < st["maxCoordinate"] < 2.2e4 and st["scaleExponent"] == -1           # below 2^(e + 21) = 2^20
    with pytest.raises(sc.Invalid, match="diverged"):
        sc.smooth(p, tri, 80, 0.3, -1.0)


def test_empty_meshes_and_no_iterations():
    p, tri = sc.grid_mesh(4, 4, jitter=0.2, seed=1)
    out, st = sc.smooth(p[:0], tri[:0], 2, 0.5, -0.53)
    assert out.shape == (0, 3) and st == dict(dict.fromkeys(sc.STAT_NAMES, 0), passes=4, maxMove=0.0, maxCoordinate=0.0)
    out, st = sc.smooth(p, tri[:0], 2, 0.5, -0.53)
    assert st["isolatedVertices"] == 16 and st["numEdges"] == 0 and out.tobytes() == p.tobytes()
    out, st = sc.smooth(p[:0], tri, 2, 0.5, -0.53)
    assert st["outOfRangeTriangles"] == 18 and out.shape == (0, 3)
    out, st = sc.smooth(p, tri, 0, 0.5, -0.53)
    assert out.tobytes() == p.tobytes() and (st["passes"], st["numEdges"], st["boundaryEdges"], st["maxMove"]) == (0, 33, 12, 0.0)
    assert st["scaleExponent"] == 1 and st["maxCoordinate"] == float(np.abs(p).max())
    zeros = np.zeros((16, 3), np.float32)
    zeros[3, 1] = -0.0
    out, st = sc.smooth(zeros, tri, 2, 0.5, -0.53, sc.CURVE)
    assert out.tobytes() == zeros.tobytes() and (st["scaleExponent"], st["maxCoordinate"], st["passes"]) == (0, 0.0, 4)


@pytest.mark.parametrize("lam, mu, mode", [(0.0, -0.5, 0), (1.5, -0.5, 0), (np.nan, -0.5, 0), (0.5, 0.1, 0), (0.5, -1.5, 0),
                                           (0.5, np.nan, 0), (0.5, -0.5, 7)])
def test_parameters_are_checked(lam, mu, mode):
    p, tri = sc.octahedron()
    with pytest.raises(sc.Invalid, match="parameters"):
        sc.smooth(p, tri, 1, lam, mu, mode)


def test_a_vertex_that_is_not_finite_is_an_error():
    p, tri = sc.octahedron()
    p[2, 1] = np.inf
    with pytest.raises(sc.Invalid, match="vertex"):
        sc.smooth(p, tri, 1, 0.5, -0.5)
