"""The CPU oracle of the long-edge split (split_cases.py) against hand cases written out literally and against what the contract
in include/mlsgpu_hip.h says must follow; test_gpu_split.py then holds the device to the oracle bit for bit."""
import numpy as np
import pytest

import split_cases as sp

MAX_ROUNDS = 64
FACTORS = (0.7, 0.4, 0.2)


def bits(rows):
    return np.asarray(rows, np.float32).view(np.uint32).tolist()


def small_meshes():
    return (sp.flat_grid(20, 20, 0.3, 1), sp.noisy_torus(40, 12, 0.004, 7), sp.fan_mesh(200, seed=1))


@pytest.fixture(scope="module")
def converged():
    """[(vertices, triangles, length, result)] for the three meshes at the three lengths."""
    out = []
    for p, tri in small_meshes():
        longest = sp.longest_edge(p, tri)
        out += [(p, tri, f * longest, sp.split(p, tri, MAX_ROUNDS, f * longest)) for f in FACTORS]
    return out


# ---------------------------------------------------------------- hand cases

def test_one_triangle_is_a_boundary_split():
    v, t, st, ends = sp.split(*sp.one_triangle(), MAX_ROUNDS, 3.5)
    assert t.tolist() == [[0, 3, 2], [3, 1, 2]] and ends.tolist() == [[0, 1]]
    assert bits(v[3]) == [0x40000000, 0, 0]                         # (2, 0, 0)
    assert st == dict(sp.empty_stats(), numVertices=3, numTriangles=1, numEdges=3, boundaryEdges=3, rounds=2, splits=1, boundarySplits=1,
                      converged=1, longBefore=1, outVertices=4, outTriangles=2, maxLengthSqBefore=16.0, maxLengthSqAfter=10.0,
                      minQualityBefore=st["minQualityBefore"], minQualityAfter=st["minQualityAfter"],
                      qualityBefore=st["qualityBefore"], qualityAfter=st["qualityAfter"])
    assert sum(st["qualityBefore"]) == 1 and sum(st["qualityAfter"]) == 2
    # the only side runs b -> a: T2 = (b, a, d), the corner b becomes m, the new row is (b, m, d)
    p, tri = sp.one_triangle()
    v, t, st, ends = sp.split(p, tri[:, [1, 0, 2]], MAX_ROUNDS, 3.5)
    assert t.tolist() == [[3, 0, 2], [1, 3, 2]] and ends.tolist() == [[0, 1]] and st["boundarySplits"] == 1


def test_long_diagonal_is_an_interior_split():
    v, t, st, ends = sp.split(*sp.long_diagonal(), MAX_ROUNDS, 2.5)
    assert t.tolist() == [[0, 4, 2], [4, 0, 3], [4, 1, 2], [1, 4, 3]] and ends.tolist() == [[0, 1]]
    assert bits(v[4]) == [0x3F800000, 0x3F800000, 0]                # (1, 1, 0)
    assert (st["interiorEdges"], st["boundaryEdges"], st["splits"], st["boundarySplits"], st["rounds"], st["converged"]) == (1, 4, 1, 0, 2, 1)
    assert (st["maxLengthSqBefore"], st["maxLengthSqAfter"], st["longBefore"], st["longAfter"]) == (8.0, 4.0, 1, 0)


def test_ties_are_broken_by_the_vertex_pair():
    # the grid cell: in every triangle the two legs tie, behind the hypotenuse; the hypotenuses 1 2 and 3 4 go first
    v, t, st, ends = sp.split(*sp.tied_pair(), 1, 0.9)
    assert ends.tolist() == [[1, 2], [3, 4]] and st["longBefore"] == 7
    assert t.tolist() == [[0, 1, 5], [1, 3, 5], [1, 6, 3], [5, 2, 0], [2, 5, 3], [4, 6, 1]]
    assert bits(v[5:]) == bits([[0.5, 0.5, 0], [1.5, 0.5, 0]])
    # one triangle whose two longest sides tie: (0, 2) < (1, 2), so 0 2 is first, and its only side runs 2 -> 0
    v, t, st, ends = sp.split(*sp.isosceles(), 1, 3.1)
    assert ends.tolist() == [[0, 2]] and t.tolist() == [[0, 1, 3], [2, 3, 1]] and st["longBefore"] == 2 and st["longAfter"] == 1
    assert bits(v[3]) == bits([0.5, 1.5, 0])
    # and whichever way the rows are turned
    p, tri = sp.isosceles()
    for turn in range(3):
        assert sp.split(p, np.roll(tri, turn, axis=1), 1, 3.1)[3].tolist() == [[0, 2]]


def test_a_fin_is_irregular_and_freezes_its_triangles():
    p, tri = sp.fin()
    v, t, st, ends = sp.split(p, tri, MAX_ROUNDS, 3.0)              # only 0 1 is long, and it is blocked
    assert t.tolist() == tri.tolist() and len(ends) == 0
    assert (st["interiorEdges"], st["boundaryEdges"], st["numEdges"]) == (0, 6, 7)
    assert (st["longBefore"], st["longAfter"], st["blockedAfter"], st["splits"], st["rounds"], st["converged"]) == (1, 1, 1, 0, 1, 1)
    st = sp.split(p, tri, MAX_ROUNDS, 2.0)[2]                       # all seven are long: 0 1 is the first side of each triangle
    assert (st["longBefore"], st["longAfter"], st["blockedAfter"], st["splits"], st["converged"]) == (7, 7, 1, 0, 1)


def test_a_pinned_triangle_stays():
    p, tri = sp.one_triangle()
    v, t, st, ends = sp.split(p, tri, MAX_ROUNDS, 1.0, pinned=np.ones(3, np.uint8))
    assert (st["blockedAfter"], st["longAfter"], st["rounds"], st["converged"], st["splits"]) == (3, 3, 1, 1, 0)
    assert t.tolist() == tri.tolist() and v.tobytes() == p.tobytes()
    st = sp.split(p, tri, MAX_ROUNDS, 1.0, pinned=[1, 0, 1])[2]     # one free end suffices; new vertices are never pinned
    assert st["converged"] == 1 and st["longAfter"] == st["blockedAfter"] == 1 and st["splits"] > 3


def test_defect_rows_keep_bits_and_place():
    p, tri = sp.defect_mesh()
    v, t, st, ends = sp.split(p, tri, MAX_ROUNDS, 0.7)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 2) and st["splits"] > 20 and st["converged"] == 1
    rows = (tri & 0xFFFFFFFF).astype(np.uint32)
    for row in (5, 77, 20, 121):
        assert t[row].tolist() == rows[row].tolist()
    assert st["outVertices"] > len(p) + 1                           # vertex V exists now, and row 5, which names it, still takes no part
    assert st["qualityAfter"] == sp.split(v, np.delete(t, (5, 77, 20, 121), axis=0), 0, 0.7)[2]["qualityBefore"]
    assert v[:len(p)].tobytes() == p.tobytes()


# ---------------------------------------------------------------- what follows from the contract

def test_converged_meshes(converged):
    rounds = []
    for p, tri, length, (v, t, st, ends) in converged:
        rounds.append(st["rounds"])
        assert st["converged"] == 1 and st["limited"] == 0 and st["longAfter"] == 0 and st["blockedAfter"] == 0
        assert st["maxLengthSqAfter"] <= np.float64(length) * np.float64(length) < st["maxLengthSqBefore"]
        assert st["outTriangles"] == st["numTriangles"] + 2 * st["splits"] - st["boundarySplits"] == len(t)
        assert st["outVertices"] == st["numVertices"] + st["splits"] == len(v) and len(ends) == st["splits"]
        assert v[:len(p)].tobytes() == p.tobytes() and (ends[:, 0] < ends[:, 1]).all()
        # every new vertex is the float midpoint of its ends, which were made before it
        assert (ends[:, 1] < len(p) + np.arange(len(ends))).all()
        v64 = v.astype(np.float64)
        assert v[len(p):].tobytes() == ((v64[ends[:, 0]] + v64[ends[:, 1]]) * 0.5).astype(np.float32).tobytes()
        before, after = sp.invariants(len(p), tri), sp.invariants(len(v), t)
        assert after == dict(before, boundaryEdges=before["boundaryEdges"] + st["boundarySplits"])
        assert abs(sp.area(v, t) / sp.area(p, tri) - 1) < 1e-6      # measured: at most 1.1e-8
    assert 3 <= min(rounds) and max(rounds) <= 12                   # the oracle counts the round that finds nothing


def test_torus_sizes_are_the_prototypes(converged):
    assert [len(r[3][1]) for r in converged[3:6]] == [2058, 5876, 23470]


def test_fixed_point_and_pure_report(converged):
    for p, tri, length, want in converged:
        v, t, st, ends = want
        again = sp.split(v, t, MAX_ROUNDS, length)
        assert again[0].tobytes() == v.tobytes() and again[1].tobytes() == t.tobytes() and len(again[3]) == 0
        assert (again[2]["splits"], again[2]["rounds"], again[2]["converged"], again[2]["longBefore"]) == (0, 1, 1, 0)
        assert again[2]["qualityBefore"] == again[2]["qualityAfter"] == st["qualityAfter"]
        report = sp.split(p, tri, 0, length)
        assert report[0].tobytes() == p.tobytes() and report[1].tolist() == tri.tolist() and len(report[3]) == 0
        expect = dict(st, rounds=0, splits=0, boundarySplits=0, converged=0, longAfter=st["longBefore"], outVertices=len(p), outTriangles=len(tri),
                      minQualityAfter=st["minQualityBefore"], maxLengthSqAfter=st["maxLengthSqBefore"], qualityAfter=st["qualityBefore"])
        assert report[2] == expect


def test_unjittered_grid_of_ties():
    p, tri = sp.grid_mesh(20, 20)
    for factor, size in zip(FACTORS, (2888, 5776, 23104)):
        v, t, st, _ = sp.split(p, tri, MAX_ROUNDS, factor * np.sqrt(2.0))
        assert st["converged"] == 1 and 2 <= st["rounds"] - 1 <= 6 and len(t) == size and st["longAfter"] == 0
        assert sp.area(v, t) == sp.area(p, tri)


def test_limit_between_two_rounds():
    p, tri = sp.flat_grid(20, 20, 0.3, 1)
    length = 0.3 * sp.longest_edge(p, tri)
    sizes = [sp.split(p, tri, r, length)[2]["outTriangles"] for r in range(5)]
    assert sizes[0] == len(tri) and all(x < y for x, y in zip(sizes, sizes[1:]))
    for limit in (sizes[3] - 1, sizes[2], sizes[2] + 1):
        v, t, st, ends = sp.split(p, tri, MAX_ROUNDS, length, limit)
        assert (st["limited"], st["converged"], st["rounds"], st["outTriangles"]) == (1, 0, 2, sizes[2])
        same = sp.split(p, tri, 2, length)
        sp.assert_same((v, t, dict(st, limited=0), ends), same)
    st = sp.split(p, tri, MAX_ROUNDS, length, len(tri))[2]
    assert (st["limited"], st["rounds"], st["splits"], st["outTriangles"]) == (1, 0, 0, len(tri))
    assert sp.split(p, tri, MAX_ROUNDS, length, sizes[3])[2]["rounds"] >= 3
    full = sp.split(p, tri, MAX_ROUNDS, length)
    sp.assert_same(sp.split(p, tri, MAX_ROUNDS, length, full[2]["outTriangles"]), full)     # the limit itself is allowed
    assert sp.split(p, tri, 2, length, sizes[3] - 1)[2]["limited"] == 0        # the rounds end first


def test_permutation_rotation_and_scaling(converged):
    for p, tri, length, want in converged[::4]:
        order = np.random.default_rng(3).permutation(len(tri))
        got = sp.split(p, tri[order], MAX_ROUNDS, length)
        assert got[2] == want[2] and got[0].tobytes() == want[0].tobytes() and got[3].tolist() == want[3].tolist()
        assert sp.triangle_set(got[1]).tolist() == sp.triangle_set(want[1]).tolist()
        got = sp.split(p, sp.rotated(tri, 4), MAX_ROUNDS, length)
        assert got[0].tobytes() == want[0].tobytes() and got[3].tolist() == want[3].tolist()
        assert sp.triangle_set(got[1]).tolist() == sp.triangle_set(want[1]).tolist()
        assert dict(got[2], **dict((k, want[2][k]) for k in sp.QUALITY_NAMES)) == want[2]
        for shift in (-7, 40, -60):
            s = np.float32(2.0) ** np.float32(shift)
            got = sp.split(p * s, tri, MAX_ROUNDS, length * float(s))
            expect = dict(want[2], maxLengthSqBefore=want[2]["maxLengthSqBefore"] * float(s) ** 2,
                          maxLengthSqAfter=want[2]["maxLengthSqAfter"] * float(s) ** 2)
            sp.assert_same(got, (want[0] * s, want[1], expect, want[3]))


def test_pinned_rim():
    p, tri = sp.flat_grid(20, 20, 0.3, 1)
    pinned = sp.rim_of(len(p), tri)
    assert pinned.sum() == 76
    v, t, st, ends = sp.split(p, tri, MAX_ROUNDS, 0.3 * sp.longest_edge(p, tri), pinned=pinned)
    assert st["converged"] == 1 and st["longAfter"] > st["blockedAfter"] > 0 and st["boundarySplits"] == 0
    rim = sp.rim_of(len(v), t)
    assert rim[:len(p)].tolist() == pinned.tolist() and rim[len(p):].sum() == 0    # the rim is as it was


def test_inputs_of_the_gpu_tests():
    p, tri = sp.fan_mesh(20_000, seed=1)
    e = p[1:].astype(np.float64) - p[0].astype(np.float64)
    st = sp.split(p, tri, MAX_ROUNDS, 0.9 * float(np.sqrt((e * e).sum(axis=1).min())))[2]
    assert st["converged"] == 1 and st["longAfter"] == 0 and st["rounds"] < 16
    p, tri = sp.noisy_torus(200, 40, 0.004, 7)
    st = sp.split(p, tri, MAX_ROUNDS, 0.6 * sp.longest_edge(p, tri))[2]
    assert st["converged"] == 1 and st["splits"] > 1000 and st["boundarySplits"] == 0


def test_parameter_errors():
    p, tri = sp.long_diagonal()
    for max_length, limit in [(0.0, 0), (-1.0, 0), (np.inf, 0), (np.nan, 0), (1.0, 1)]:
        with pytest.raises(sp.Invalid, match="parameters"):
            sp.split(p, tri, 1, max_length, limit)
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[2, 1] = bad
        with pytest.raises(sp.Invalid, match="vertex"):
            sp.split(q, tri, 1, 1.0)
    assert sp.split(p, tri, 1, 1.0, 2)[2]["limited"] == 1
