"""The contract of the hole filling (include/mlsgpu_hip.h) on the CPU oracle of fill_cases.py: the hand cases, the identities
and the invariances the contract promises, and what filling does to the topology report."""
import numpy as np
import pytest

import fill_cases as fc
import smooth_cases as sc
import topology_cases as tc


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# the issue's fixture: a jittered 40 x 40 grid with four rectangular holes of 4, 10, 8 and 32 sides, unused vertices gone
HOLES = [(5, 5, 1, 1), (10, 20, 2, 3), (20, 8, 2, 2), (28, 25, 8, 8)]


@pytest.fixture(scope="module")
def sheet():
    return fc.punched(40, 40, HOLES, jitter=0.2, seed=3, compact=True)


# ---------------------------------------------------------------- hand cases

def test_single_triangle_gets_a_cap():
    p = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 3]], np.float32)
    v, t, st = fc.fill(p, [[0, 1, 2]], 3)
    assert v.tolist() == p.tolist() + [[1.0, 1.0, 1.0]]
    assert t.tolist() == [[0, 1, 2], [1, 0, 3], [2, 1, 3], [0, 2, 3]]
    assert st == dict(numVertices=3, numTriangles=1, outOfRangeTriangles=0, degenerateTriangles=0, boundaryEdges=3, irregularEdges=0,
                      loops=1, filledLoops=1, longLoops=0, pinnedLoops=0, filledEdges=3, longestLoop=3, outVertices=4,
                      outTriangles=4, scaleExponent=1)
    after = tc.count_all(4, t)
    assert after["manifold"] == 1 and after["numBoundaries"] == 0 and after["eulerCharacteristic"] == 2


def test_octahedron_without_a_face():
    p, tri = sc.octahedron()
    v, t, st = fc.fill(p, tri[1:], 8)                           # (0, 2, 4) is gone
    assert (st["boundaryEdges"], st["loops"], st["filledLoops"], st["filledEdges"], st["longestLoop"]) == (3, 1, 1, 3, 3)
    assert t[:7].tolist() == tri[1:].tolist()
    # the sides 0 -> 2, 2 -> 4, 4 -> 0 are missing: their opposites bound the hole, and the new triangles carry them
    assert t[7:].tolist() == [[4, 0, 6], [0, 2, 6], [2, 4, 6]]
    np.testing.assert_array_equal(bits(v[:6]), bits(p))
    assert v[6].tolist() == [np.float32(1 / 3)] * 3 and st["scaleExponent"] == 0
    after = tc.count_all(7, t)
    assert after["manifold"] == 1 and after["numBoundaries"] == 0 and after["eulerCharacteristic"] == 2


def test_closed_torus_is_left_alone():
    p, tri = fc.torus_mesh(7, 5, 0.5, 0.125)
    v, t, st = fc.fill(p, tri, 100)
    np.testing.assert_array_equal(bits(v), bits(p))
    assert t.tolist() == tri.tolist() and t.dtype == np.uint32
    assert [st[k] for k in fc.STAT_NAMES[2:12]] == [0] * 10 and st["outVertices"] == 35 and st["outTriangles"] == 70


def test_empty_meshes():
    v, t, st = fc.fill(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), 3)
    assert v.shape == (0, 3) and t.shape == (0, 3) and not any(st.values())
    v, t, st = fc.fill(np.zeros((0, 3), np.float32), [[0, 1, 2], [5, 5, 5]], 3)
    assert st["outOfRangeTriangles"] == 2 and st["outTriangles"] == 2 and t.tolist() == [[0, 1, 2], [5, 5, 5]]
    v, t, st = fc.fill(np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int64), 3)
    assert st["outVertices"] == 4 and st["scaleExponent"] == 0
    v, t, st = fc.fill(np.zeros((3, 3), np.float32), [[0, 1, 2]], 3)            # all-zero positions: e = 0, a cap at zero
    assert st["scaleExponent"] == 0 and st["filledLoops"] == 1 and v[3].tolist() == [0, 0, 0]


def test_refusals():
    p, tri = fc.grid_mesh(3, 3)
    for max_edges in (2, 2 ** 20 + 1, 0):
        with pytest.raises(fc.Invalid):
            fc.fill(p, tri, max_edges)
    q = p.copy()
    q[8, 1] = np.nan                                            # a vertex no triangle needs to use
    with pytest.raises(fc.Invalid):
        fc.fill(q, tri[:2], 8)
    fc.fill(p, tri, 2 ** 20)


def test_defects_take_no_part_and_stay():
    p, tri = fc.punched(6, 6, [(2, 2, 1, 1)])
    extra = np.array([[0, 1, 36], [7, 7, 8], [0xFFFFFFFF, 2, 3], [9, 9, 9]], np.int64)
    both = np.concatenate([extra[:2], tri, extra[2:]])
    v, t, st = fc.fill(p, both, 4)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 2)
    assert t[:len(both)].tolist() == both.tolist()
    assert (st["loops"], st["filledLoops"], st["longLoops"], st["filledEdges"]) == (2, 1, 1, 4)
    # a side used twice in one direction is no boundary side: its component has a vertex with no side out
    twice = np.concatenate([tri, [[0, 6, 36 - 1]]])             # 0 -> 6 is the rim's own side (triangle (0, 6, 7))
    assert fc.boundary_sides(36, tri)[0].tolist().count(0) == 1
    st2 = fc.fill(p, twice, 2 ** 20)[2]
    assert st2["irregularEdges"] > 0 and st2["loops"] == 1 and st2["filledLoops"] == 1
    # every triangle twice: every side occurs twice, nothing is boundary
    st3 = fc.fill(p, np.concatenate([tri, tri[::-1]]), 2 ** 20)[2]
    assert st3["boundaryEdges"] == 0 and st3["loops"] == 0


def test_classification_differs_from_the_topology_report():
    p, tri = tc.classification_trap()
    tc.assert_trap_report(tc.count_all(len(p), tri))                # there: one out of range, two degenerate
    _, st = sc.smooth(p, tri, 1, 0.5, -0.53)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 1)         # smoothing: (1, 1, 7) is out of range
    v, t, st = fc.fill(p, tri, 8)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 1)         # and so it is here
    assert (st["boundaryEdges"], st["loops"], st["filledLoops"], st["filledEdges"]) == (4, 1, 1, 4)
    assert t[:5].tolist() == tri.tolist() and v[4].tolist() == [0.5, 0.5, 0.0]      # the bad ones stay, and take no part


def test_figure_eight_is_irregular():
    p, tri = fc.figure_eight()
    v, t, st = fc.fill(p, tri, 2 ** 20)
    assert st["irregularEdges"] == 8 and st["loops"] == 1 and st["filledLoops"] == 1 and st["filledEdges"] == 20
    assert st["boundaryEdges"] == 28
    # the two holes are still there: the sides around them have no opposite
    assert len(fc.boundary_sides(len(v), t)[0]) == 8


# ---------------------------------------------------------------- identities and topology

@pytest.mark.parametrize("max_edges", [3, 4, 8, 9, 10, 32, 2 ** 20])
def test_identities_and_topology(sheet, max_edges):
    p, tri = sheet
    before = tc.count_all(len(p), tri)
    assert before["manifold"] == 1 and before["numBoundaries"] == 5 and before["eulerCharacteristic"] == -3
    assert before["numVertices"] == 40 * 40 - 2 - 1 - 49
    v, t, st = fc.fill(p, tri, max_edges)
    sizes = sorted([4, 10, 8, 32, 4 * 39])
    assert st["loops"] == 5 == st["filledLoops"] + st["longLoops"] + st["pinnedLoops"] and st["pinnedLoops"] == 0
    assert st["longestLoop"] == 156 and st["irregularEdges"] == 0 and st["boundaryEdges"] == sum(sizes)
    filled = [n for n in sizes if n <= max_edges]
    assert st["filledLoops"] == len(filled) and st["filledEdges"] == sum(filled) and st["longLoops"] == 5 - len(filled)
    after = tc.count_all(len(v), t)
    assert after["manifold"] == 1
    assert after["numBoundaries"] == 5 - len(filled)
    assert after["boundaryEdges"] == before["boundaryEdges"] - sum(filled)
    assert after["eulerCharacteristic"] == -3 + len(filled)
    np.testing.assert_array_equal(bits(v[:len(p)]), bits(p))
    assert t[:len(tri)].tolist() == tri.tolist()
    new = t[len(tri):].astype(np.int64)
    assert (np.diff(new[:, 1]) > 0).all()                       # step 10: ascending a
    assert (np.diff(new[:, 2][np.argsort(new[:, 2], kind="stable")]) >= 0).all() and (new[:, 2] >= len(p)).all()
    # step 8: the loops are numbered by their smallest vertex
    smallest = [new[new[:, 2] == len(p) + j, 1].min() for j in range(len(filled))]
    assert smallest == sorted(smallest)
    # a second round finds nothing left that it may fill
    again = fc.fill(v, t, max_edges)[2]
    assert again["filledLoops"] == 0 and again["loops"] == 5 - len(filled)


def test_the_issues_three_stages(sheet):
    p, tri = sheet
    rows = []
    for max_edges in (None, 10, 2 ** 20):
        v, t = (p, tri) if max_edges is None else fc.fill(p, tri, max_edges)[:2]
        r = tc.count_all(len(v), t)
        rows.append((r["manifold"], r["numBoundaries"], r["eulerCharacteristic"]))
    assert rows == [(1, 5, -3), (1, 2, 0), (1, 0, 2)]


def test_new_vertex_is_the_fixed_point_mean(sheet):
    p, tri = sheet
    v, t, st = fc.fill(p, tri, 32)
    e = st["scaleExponent"]
    assert e == 5                                               # 32 <= 39.2 < 64
    new = t[len(tri):].astype(np.int64)
    for j in range(st["filledLoops"]):
        ring = new[new[:, 2] == len(p) + j, 1]
        S = sum(np.rint(np.ldexp(p[a].astype(np.float64), 30 - e)).astype(np.int64) for a in ring)
        want = np.ldexp(S.astype(np.float64) / len(ring), e - 30).astype(np.float32)
        assert bits(v[len(p) + j]).tolist() == bits(want).tolist()
        assert np.abs(v[len(p) + j] - p[ring].astype(np.float64).mean(axis=0)).max() < 2.0 ** (e - 22)


def test_torus_with_holes():
    p, tri = fc.punched_torus(12, 9, [(1, 1, 1, 1), (5, 3, 2, 2)])
    before = tc.count_all(len(p), tri)
    assert before["manifold"] == 1 and before["numBoundaries"] == 2
    v, t, st = fc.fill(p, tri, 8)
    after = tc.count_all(len(v), t)
    assert st["filledLoops"] == 2 and st["filledEdges"] == 12 and after["manifold"] == 1 and after["numBoundaries"] == 0
    assert after["eulerCharacteristic"] == 0


# ---------------------------------------------------------------- invariances

def test_renumbering_keeps_the_soup(sheet):
    p, tri = sheet
    want = fc.soup(*fc.fill(p, tri, 12)[:2])
    for seed in (1, 2):
        q, tri2, _ = fc.renumbered(p, tri, seed)
        v, t, st = fc.fill(q, tri2, 12)
        assert st["filledLoops"] == 3 and fc.soup(v, t) == want
    order = np.random.default_rng(5).permutation(len(tri))     # the order of the triangles moves the copied prefix only
    v, t, _ = fc.fill(p, tri[order], 12)
    assert fc.soup(v, t) == want and t[len(tri):].tolist() == fc.fill(p, tri, 12)[1][len(tri):].tolist()


@pytest.mark.parametrize("shift", [-60, -20, 7, 80])
def test_scaling_by_a_power_of_two_is_exact(sheet, shift):
    p, tri = sheet
    v, t, st = fc.fill(p, tri, 32)
    scaled = np.ldexp(p, shift)
    assert np.array_equal(np.ldexp(scaled.astype(np.float64), -shift), p.astype(np.float64))       # nothing was lost on the way
    v2, t2, st2 = fc.fill(scaled, tri, 32)
    assert st2["scaleExponent"] == st["scaleExponent"] + shift and t2.tolist() == t.tolist()
    assert np.array_equal(np.ldexp(v2.astype(np.float64), -shift), v.astype(np.float64))
    assert dict(st2, scaleExponent=0) == dict(st, scaleExponent=0)


def test_long_comes_before_pinned(sheet):
    p, tri = sheet
    fa, _, _, _ = fc.boundary_sides(len(p), tri)
    none = fc.fill(p, tri, 12)[2]
    assert (none["filledLoops"], none["longLoops"], none["pinnedLoops"]) == (3, 2, 0)
    pinned = np.zeros(len(p), bool)
    pinned[fa] = True                                           # every boundary vertex
    st = fc.fill(p, tri, 12, pinned)[2]
    assert (st["filledLoops"], st["longLoops"], st["pinnedLoops"]) == (0, 2, 3) and st["outTriangles"] == len(tri)
    st = fc.fill(p, tri, 2 ** 20, pinned)[2]
    assert (st["filledLoops"], st["longLoops"], st["pinnedLoops"]) == (0, 0, 5)
    one = np.zeros(len(p), bool)
    one[fa.min()] = True                                        # vertex 0, on the rim
    st = fc.fill(p, tri, 2 ** 20, one)[2]
    assert (st["filledLoops"], st["longLoops"], st["pinnedLoops"]) == (4, 0, 1)
    inner = np.ones(len(p), bool)
    inner[fa] = False                                           # pinned vertices that are on no boundary change nothing
    assert fc.fill(p, tri, 12, inner)[2] == none
