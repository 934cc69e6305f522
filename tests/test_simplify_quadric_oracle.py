"""The CPU oracle of quadric-error vertex placement (simplify_quadric_cases.simplify_quadric) against the contract in
include/mlsgpu_hip.h and against geometry: what the device is then compared with bit for bit (test_gpu_simplify_quadric.py)."""
import numpy as np
import pytest

import simplify_cases as sc
import simplify_quadric_cases as qc

CUBE = dict(n=24, L=24.0, jitter=0.3, cell=3.7, origin=(-1.3, -2.1, -0.7))
TORI = [(1.7, 0.0), (3.1, 0.0), (1.7, 0.02), (3.1, 0.02)]


def torus(sigma, seed=3):
    p, tri = sc.torus_mesh(96, 48, 20.0, 6.0)
    if sigma:
        p = (p.astype(np.float64) + np.random.default_rng(seed).normal(0.0, sigma, p.shape)).astype(np.float32)
    return p, tri


def cases():
    yield sc.grid_mesh(4, 4) + ((-0.5, -0.5, -0.5), 2.0)
    yield sc.grid_mesh(40, 30, jitter=0.3, seed=1) + ((-1.0, -1.0, -1.0), 3.0)
    yield qc.cube_mesh(8, 8.0, 0.3, 2) + ((-0.9, -0.4, -1.1), 2.3)
    yield sc.torus_mesh(97, 6, 10.0, 0.1, windings=2) + ((-12.5, -12.5, -12.5), 2.5)
    yield qc.wedge_mesh()
    yield qc.line_mesh() + ((-0.2, 0.0, 0.0), 1.0)
    yield qc.flat_and_grid_mesh() + ((-0.2, -1.0, 0.0), 1.0)


@pytest.mark.parametrize("case", range(7))
def test_triangles_and_shared_statistics_are_the_mean_variants(case):
    p, tri, origin, cell = list(cases())[case]
    v, t, st = qc.simplify_quadric(p, tri, origin, cell)
    mv, mt, mst = sc.simplify(p, tri, origin, cell)
    np.testing.assert_array_equal(t, mt)
    assert v.shape == mv.shape
    assert dict((k, st[k]) for k in sc.STAT_NAMES) == mst


def test_degenerate_meshes_fall_back_to_the_mean_bit_for_bit():
    p, tri = qc.line_mesh()
    v, t, st = qc.simplify_quadric(p, tri, (-0.2, 0.0, 0.0), 1.0)
    mv, _, _ = sc.simplify(p, tri, (-0.2, 0.0, 0.0), 1.0)
    assert v.tobytes() == mv.tobytes()
    assert st["flatVertices"] > 0 and st["solvedVertices"] == st["escapedVertices"] == 0 and st["scaleExponent"] == 0
    # M != 0, and clusters whose quadric is zero
    p, tri = qc.flat_and_grid_mesh()
    d = {}
    v, t, st = qc.simplify_quadric(p, tri, (-0.2, -1.0, 0.0), 1.0, details=d)
    mv, _, _ = sc.simplify(p, tri, (-0.2, -1.0, 0.0), 1.0)
    assert st["flatVertices"] > 0 and st["solvedVertices"] > 0
    flat = d["kind"] == 2
    assert v[flat].tobytes() == mv[flat].tobytes()
    assert (v[flat][:, 2] < 10).all() and (v[d["kind"] == 1][:, 2] > 10).all()


def test_single_member_clusters_are_kept():
    p, tri = sc.grid_mesh(40, 30, jitter=0.3, seed=1)
    d = {}
    v, t, st = qc.simplify_quadric(p, tri, (-1.0, -1.0, -1.0), 1.3, details=d)
    single = d["kind"] == 0
    assert single.sum() > 100 and (d["kind"] == 1).sum() > 100
    have = set(map(bytes, p.view(np.uint8).reshape(len(p), 12)))
    assert all(bytes(row) in have for row in v[single].view(np.uint8).reshape(-1, 12))


@pytest.mark.parametrize("shear", [0.0, 0.37])
def test_a_plane_keeps_the_means_position_along_it(shear):
    """A jittered grid in the plane z = 5 + shear * x: the quadric has rank 1, the output lies in the plane and, inside it,
    where the mean lies."""
    p, tri = sc.grid_mesh(40, 30, jitter=0.3, seed=6)
    p[:, 2] = 5.0
    p = p.astype(np.float64)
    p[:, 2] += shear * p[:, 0]
    p = p.astype(np.float32)
    origin, cell = (-1.1, -0.9, -0.3), 2.9
    d = {}
    v, t, st = qc.simplify_quadric(p, tri, origin, cell, details=d)
    mv, _, _ = sc.simplify(p, tri, origin, cell)
    solved = d["kind"] == 1
    assert solved.sum() > 50 and st["escapedVertices"] == st["flatVertices"] == 0
    v, mv = v[solved].astype(np.float64), mv[solved].astype(np.float64)
    normal = np.array([-shear, 0.0, 1.0]) / np.sqrt(1.0 + shear * shear)
    off_plane = (v[:, 2] - (5.0 + shear * v[:, 0])) / np.sqrt(1.0 + shear * shear)
    assert np.abs(off_plane).max() <= 1e-6 * cell
    # the mean lies in the plane too (to float32's rounding): compare the components along the plane
    diff = v - mv
    in_plane = diff - np.outer(diff @ normal, normal)
    assert np.abs(in_plane).max() <= 1e-6 * cell


def test_invariance_is_exact():
    p, tri = qc.cube_mesh(8, 8.0, 0.3, 2)
    origin, cell = (-0.875, -0.375, -1.125), 2.25
    want = qc.simplify_quadric(p, tri, origin, cell)
    assert want[2]["solvedVertices"] > 20
    qc.assert_same(qc.simplify_quadric(p, qc.permuted_triangles(tri, 1), origin, cell), want)
    qc.assert_same(qc.simplify_quadric(*qc.renumbered(p, tri, 2), origin, cell), want)
    v8, t8, st8 = qc.simplify_quadric(p * np.float32(8), tri, tuple(8 * x for x in origin), 8 * cell)
    assert st8 == want[2]
    np.testing.assert_array_equal(t8, want[1])
    assert v8.tobytes() == (want[0] * np.float32(8)).tobytes()


@pytest.mark.parametrize("seed", [0, 1])
def test_creases_of_a_cube(seed):
    """The RMS distance of the multi-member vertices to the cube is at most 1/64 of the mean variant's: with mu = 2^-10 tr a
    balanced right-angled crease keeps about 2^-9 of the mean's offset, and 1/64 leaves a factor of 8."""
    p, tri = qc.cube_mesh(CUBE["n"], CUBE["L"], CUBE["jitter"], seed)
    d = {}
    v, t, st = qc.simplify_quadric(p, tri, CUBE["origin"], CUBE["cell"], details=d)
    mv, _, _ = sc.simplify(p, tri, CUBE["origin"], CUBE["cell"])
    multi = d["kind"] != 0
    assert multi.sum() > 200
    assert st["escapedVertices"] + st["flatVertices"] == 0          # not by falling back
    quadric = np.sqrt((qc.cube_distance(v[multi], CUBE["L"]) ** 2).mean())
    mean = np.sqrt((qc.cube_distance(mv[multi], CUBE["L"]) ** 2).mean())
    print("cube seed %d: rms to the cube, in cells: mean %.5f quadric %.6f ratio %.0f; max mean %.4f quadric %.5f"
          % (seed, mean / CUBE["cell"], quadric / CUBE["cell"], mean / quadric,
             qc.cube_distance(mv[multi], CUBE["L"]).max() / CUBE["cell"], qc.cube_distance(v[multi], CUBE["L"]).max() / CUBE["cell"]))
    assert quadric <= mean / 64


@pytest.mark.parametrize("cell,sigma", TORI)
def test_a_smooth_surface_is_not_made_worse(cell, sigma):
    """Quadric vertices sit on the tangent envelope, just outside the torus, means just inside: at most twice the mean's RMS
    distance, and at most 2 % of the multi-member clusters fall back."""
    p, tri = torus(sigma)
    origin = (-27.3, -27.1, -6.9)
    d = {}
    v, t, st = qc.simplify_quadric(p, tri, origin, cell, details=d)
    mv, _, _ = sc.simplify(p, tri, origin, cell)
    multi = d["kind"] != 0
    quadric = np.sqrt((qc.torus_distance(v[multi], 20.0, 6.0) ** 2).mean())
    mean = np.sqrt((qc.torus_distance(mv[multi], 20.0, 6.0) ** 2).mean())
    fallbacks = st["escapedVertices"] + st["flatVertices"]
    print("torus cell %.1f sigma %.2f: rms mean %.5f quadric %.5f ratio %.2f; fallbacks %d of %d"
          % (cell, sigma, mean, quadric, quadric / mean, fallbacks, multi.sum()))
    assert multi.sum() > 400
    assert quadric <= 2 * mean
    assert fallbacks <= 0.02 * multi.sum()


def test_fallbacks_are_reached():
    p, tri, origin, cell = qc.wedge_mesh()
    d = {}
    v, t, st = qc.simplify_quadric(p, tri, origin, cell, details=d)
    mv, _, _ = sc.simplify(p, tri, origin, cell)
    assert st["escapedVertices"] >= 1 and st["solvedVertices"] >= 1
    escaped = d["kind"] == 3
    assert v[escaped].tobytes() == mv[escaped].tobytes()
    assert (np.abs(d["x"][escaped]) > 0.5).any(axis=1).all()
    p, tri = qc.line_mesh()
    assert qc.simplify_quadric(p, tri, (-0.2, 0.0, 0.0), 1.0)[2]["flatVertices"] >= 1


@pytest.mark.parametrize("case", range(7))
def test_the_solution_is_no_worse_than_the_mean(case):
    """x^T (A + mu I) x - 2 r^T x at the solution against the same at the mean, from the oracle's own sums."""
    p, tri, origin, cell = list(cases())[case]
    d = {}
    qc.simplify_quadric(p, tri, origin, cell, details=d)
    solved = d["kind"] == 1
    A = d["A"][solved].astype(np.float64)
    full = np.stack([A[:, [0, 1, 2]], A[:, [1, 3, 4]], A[:, [2, 4, 5]]], axis=1) + d["mu"][solved][:, None, None] * np.eye(3)

    def objective(x):
        return np.einsum("ni,nij,nj->n", x, full, x) - 2 * np.einsum("ni,ni->n", d["r"][solved], x)

    at_x, at_mean = objective(d["x"][solved]), objective(d["mean"][solved])
    scale = np.abs(at_x) + np.abs(at_mean) + np.einsum("ni,nij,nj->n", d["mean"][solved], full, d["mean"][solved])
    assert (at_x <= at_mean + 1e-9 * scale).all()
