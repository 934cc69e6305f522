"""The deviation oracle (deviation_cases.deviation) against hand cases with exact answers, against its own brute force, against
exact rational arithmetic, and under the invariances the contract promises.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import deviation_cases as dc
import fill_cases as fc
import simplify_cases as sc
import topology_cases as tc


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---------------------------------------------------------------- hand cases

@pytest.mark.parametrize("case", dc.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, p, v, t, D = case
    d, near, st = dc.deviation(p, v, t, D)
    if name == "twice":
        assert d.tolist() == [4.0, np.inf] and near.tolist() == [0, dc.NO_TRIANGLE]
        assert (st["within"], st["beyond"], st["farthestPoint"], st["maxDistance2"]) == (1, 1, 0, 4.0)
        return
    assert d.tolist() == [dc.HAND_ANSWERS[name]] and near.tolist() == [0]
    assert (st["within"], st["beyond"], st["farthestPoint"], st["farthestChunk"]) == (1, 0, 0, 0)
    assert st["maxDistance2"] == dc.HAND_ANSWERS[name] and st["limit2"] == D * D and sum(st["histogram"]) == 1
    assert dc.mean_square(st) == dc.HAND_ANSWERS[name]          # a small integer times 2^(30 - e) is an integer


def test_face_is_infinite_where_the_segments_answer():
    """A zero-area triangle has nn == 0: face() is +infinity whatever the point, and d2 is still finite."""
    for name in ("collinear", "coincident"):
        _, p, v, t, _ = [c for c in dc.hand_cases() if c[0] == name][0]
        a, b, c = (v[t[0, k]].astype(np.float64)[None] for k in range(3))
        with np.errstate(all="ignore"):
            assert dc._face(*(tuple(x.T) for x in (p.astype(np.float64), a, b, c))).tolist() == [np.inf]
        assert np.isfinite(dc.d2(p, a, b, c)).all()


def test_the_limit_is_within_and_lands_in_the_last_bin():
    p, v, t = [[1, 1, 2]], dc.RIGHT, [[0, 1, 2]]                # distance 2 exactly
    d, near, st = dc.deviation(p, v, t, 2.0)
    assert d.tolist() == [4.0] and st["within"] == 1 and st["histogram"] == [0] * 15 + [1]
    assert (st["sumQ"], st["scaleExponent"]) == (2 ** 30, 2)    # q = 4 * 2^(30 - 2), the largest a q gets is 2^31
    below = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    d, near, st = dc.deviation(p, v, t, below)
    assert d.tolist() == [np.inf] and near.tolist() == [dc.NO_TRIANGLE]
    assert (st["within"], st["beyond"], st["farthestPoint"], st["maxDistance2"], st["sumQ"]) == (0, 1, dc.NO_POINT, 0.0, 0)
    # the bins have their edges at k D / 16
    heights = np.arange(0, 17, dtype=np.float32)                # over the face, at z = 0 .. 16
    q = np.stack([np.ones(17), np.ones(17), heights], axis=1)
    d, _, st = dc.deviation(q, v, t, 16.0)
    assert d.tolist() == (heights.astype(np.float64) ** 2).tolist()
    assert st["histogram"] == [1] * 15 + [2] and st["farthestPoint"] == 16


def test_classification_trap():
    """An index >= V wins over a vertex twice (meshpost.hpp's defectOf), unlike the topology report's order."""
    p, tri = tc.classification_trap()
    d, near, st = dc.deviation(p, p, tri, 1.0)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 1)
    assert d.tolist() == [0.0] * len(p) and set(near.tolist()) <= {0, 1}


def test_empty_inputs():
    p, tri = fc.grid_mesh(4, 4)
    none = np.zeros((0, 3), np.float32)
    d, near, st = dc.deviation(none, p, tri, 2.0)
    want = dict.fromkeys(dc.STAT_NAMES, 0)
    want.update(numVertices=16, numTriangles=18, farthestPoint=dc.NO_POINT, histogram=[0] * 16, maxDistance2=0.0, limit2=4.0)
    assert st == want and len(d) == 0 and len(near) == 0
    bad = tri.copy()
    bad[3, 1] = 16
    assert dc.deviation(none, p, bad, 2.0)[2]["outOfRangeTriangles"] == 1     # the triangle counts are still made
    for target in ((none, tri), (p, tri[:0]), (p, np.full((5, 3), 7))):
        d, near, st = dc.deviation(p, *target, 2.0)
        assert st["beyond"] == 16 and st["within"] == 0 and np.isinf(d).all() and (near == dc.NO_TRIANGLE).all()
        assert st["scaleExponent"] == 2 and st["farthestPoint"] == dc.NO_POINT
    assert dc.deviation(p, none, tri, 2.0)[2]["outOfRangeTriangles"] == 18


def test_errors():
    p, tri = fc.grid_mesh(4, 4)
    for D in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(dc.Invalid, match="max distance"):
            dc.deviation(p, p, tri, D)
    q = p.copy()
    q[3, 1] = np.nan
    with pytest.raises(dc.Invalid, match="point"):
        dc.deviation(q, p, tri, 1.0)
    with pytest.raises(dc.Invalid, match="vertex"):
        dc.deviation(p, q, tri, 1.0)


# ---------------------------------------------------------------- the pruned path

def random_case(seed, points, triangles, size=0.2):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(0, 1, (triangles, 1, 3))
    v = (centre + rng.uniform(-size, size, (triangles, 3, 3))).reshape(-1, 3).astype(np.float32)
    return rng.uniform(-0.1, 1.1, (points, 3)).astype(np.float32), v, np.arange(3 * triangles).reshape(-1, 3)


@pytest.mark.parametrize("D", [0.02, 0.15, 5.0])
def test_pruned_path_is_brute_force(D):
    p, v, t = random_case(5, 1000, 1000)
    t = dc.sprinkled(t, len(v))
    brute = dc.deviation(p, v, t, D, prune=False)
    dc.assert_same(dc.deviation(p, v, t, D, prune=True), brute)
    if D == 0.02:
        assert brute[2]["within"] > 100 and brute[2]["beyond"] > 100 and brute[2]["outOfRangeTriangles"] > 50


def test_pruned_path_with_one_giant_triangle():
    """The oracle's grid doubles its cell when one triangle's box would fill it."""
    p, v, t = random_case(6, 800, 800, size=0.01)
    v = np.concatenate([v, [[-50, -50, -50], [60, -40, 55], [-45, 70, 60]]]).astype(np.float32)
    t = np.concatenate([t, [[len(v) - 3, len(v) - 2, len(v) - 1]]])
    dc.assert_same(dc.deviation(p, v, t, 0.004, prune=True), dc.deviation(p, v, t, 0.004, prune=False))


# ---------------------------------------------------------------- d2 against exact arithmetic

def exact_d2(p, a, b, c):
    """The squared distance from p to the triangle a b c over the rationals: the smallest of the three segments' and, where
    the point projects into the face, the face's."""
    F = Fraction

    def sub(u, v):
        return [x - y for x, y in zip(u, v)]

    def dot(u, v):
        return sum((x * y for x, y in zip(u, v)), F(0))

    def cross(u, v):
        return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]

    def seg(a, b):
        u, w = sub(b, a), sub(p, a)
        L = dot(u, u)
        s = min(max(dot(w, u) / L, F(0)), F(1)) if L else F(0)
        r = [x - s * y for x, y in zip(w, u)]
        return dot(r, r)

    p, a, b, c = ([F(int(x)) for x in q] for q in (p, a, b, c))
    best = min(seg(a, b), seg(b, c), seg(c, a))
    n = cross(sub(b, a), sub(c, a))
    nn = dot(n, n)
    inside = nn > 0 and all(dot(cross(sub(y, x), sub(p, x)), n) >= 0 for x, y in ((a, b), (b, c), (c, a)))
    return min(best, dot(sub(p, a), n) ** 2 / nn) if inside else best


# Measured on the 400 pairs below: the largest relative error of d2 is 3.54e-15, sixteen roundings' worth.  Every operation
# before a division is exact on these integers (|products| < 2^53), so the contract's region test is the exact one; the error
# is that of s = dot(w, u) / L, which r = w - s u carries into a difference of near-equal numbers where the point lies much
# closer to the side than to the side's first corner.  The bound is the measured figure with a margin of four, 2^-46 = 1.4e-14.
RELATIVE_BOUND = 2.0 ** -46


def test_d2_against_exact_arithmetic():
    rng = np.random.default_rng(17)
    q = rng.integers(-9, 10, (400, 4, 3))
    q[::10, 2] = q[::10, 1]                                     # coincident corners
    q[5::10, 3] = 2 * q[5::10, 2] - q[5::10, 1]                 # collinear corners
    got = dc.d2(*(q[:, k] for k in range(4)))
    worst = 0.0
    for row, g in zip(q, got):
        want = exact_d2(*row)
        if want == 0:
            assert g == 0.0
            continue
        worst = max(worst, abs(float((Fraction(float(g)) - want) / want)))
    print("largest relative error of d2 over 400 integer pairs: %.3g" % worst)
    assert worst <= RELATIVE_BOUND


# ---------------------------------------------------------------- invariances

@pytest.fixture(scope="module")
def soup():
    p, v, t = random_case(9, 700, 600)
    return p, v, dc.sprinkled(t, len(v)), dc.deviation(p, v, dc.sprinkled(t, len(v)), 0.12)


def test_permuting_the_triangles(soup):
    p, v, t, (d, near, st) = soup
    order = np.random.default_rng(1).permutation(len(t))
    d2, near2, st2 = dc.deviation(p, v, t[order], 0.12)
    assert bits(d2).tolist() == bits(d).tolist() and st2 == st
    hit = near != dc.NO_TRIANGLE
    assert (near2 != dc.NO_TRIANGLE).tolist() == hit.tolist() and (order[near2[hit]] == near[hit]).all()   # no ties in a random soup


def test_permuting_the_points(soup):
    p, v, t, (d, near, st) = soup
    order = np.random.default_rng(2).permutation(len(p))
    d2, near2, st2 = dc.deviation(p[order], v, t, 0.12)
    assert bits(d2).tolist() == bits(d[order]).tolist() and near2.tolist() == near[order].tolist()
    moved = dict(st, farthestPoint=int(np.flatnonzero(order == st["farthestPoint"])[0]))
    assert st2 == moved


@pytest.mark.parametrize("doublings", [-40, 3, 50])
def test_scaling_by_a_power_of_two(soup, doublings):
    p, v, t, (d, near, st) = soup
    f = np.float32(2.0 ** doublings)
    d2, near2, st2 = dc.deviation(p * f, v * f, t, np.float32(0.12) * f)
    assert bits(d2).tolist() == bits(d * 4.0 ** doublings).tolist() and near2.tolist() == near.tolist()
    want = dict(st, scaleExponent=st["scaleExponent"] + 2 * doublings, maxDistance2=st["maxDistance2"] * 4.0 ** doublings,
                limit2=st["limit2"] * 4.0 ** doublings)
    assert st2 == want


def test_twice_the_mesh_names_the_lower_copy(soup):
    p, v, t, (d, near, st) = soup
    d2, near2, st2 = dc.deviation(p, v, np.concatenate([t, t]), 0.12)
    assert bits(d2).tolist() == bits(d).tolist() and near2.tolist() == near.tolist()


# ---------------------------------------------------------------- natural use

def test_a_clustered_grid_stays_within_a_cluster_diameter():
    """simplify_cases' clustering at cell 3 of a 60 x 60 jittered grid: a cluster's vertices and their mean lie in one cell, so
    3 sqrt(3) bounds both directions.  The GPU test asserts the same counts; here the oracle alone shows that they hold."""
    p, tri = fc.grid_mesh(60, 60, jitter=0.3, seed=11)
    sv, stri, _ = sc.simplify(p, tri, (-1.0, -1.0, -1.0), 3.0)
    assert 300 < len(sv) < len(p) // 4
    D = np.float32(3.0 * np.sqrt(3.0))
    moved, lost = dc.deviation(sv, p, tri, D)[2], dc.deviation(p, sv, stri, D)[2]
    for st, n in ((moved, len(sv)), (lost, len(p))):
        assert st["within"] == st["numPoints"] == n and st["beyond"] == 0 and st["maxDistance2"] > 0 and sum(st["histogram"]) == n
        assert 0 < dc.mean_square(st) <= st["maxDistance2"] < st["limit2"]
    assert dc.combined([moved, lost])["within"] == len(sv) + len(p)
