"""The CPU oracle of the short-edge collapse (collapse_cases.collapse) on cases small enough to check by hand, the properties the
header states held against the topology oracle, and the convergence of the inputs that test_gpu_collapse.py uses."""
import numpy as np
import pytest

import collapse_cases as cc
import flip_cases as fc
import normals_cases as nc
import smooth_cases as sc

MAX_ROUNDS = 64


def counts(st, *names):
    return tuple(st[n] for n in names)


# ---------------------------------------------------------------- hand cases

def test_interior_pair_goes_to_its_midpoint():
    p, tri = cc.disk()
    assert cc.invariants(len(p), tri)["manifold"] == 1
    v, t, st, src = cc.collapse(p, tri, MAX_ROUNDS, 0.05)
    assert counts(st, "numEdges", "interiorEdges", "fixedVertices", "shortBefore", "shortAfter", "blockedAfter") == (43, 35, 8, 1, 0, 0)
    assert counts(st, "rounds", "collapses", "converged", "unusedVertices", "outVertices", "outTriangles") == (2, 1, 1, 1, 17, 24)
    assert st["minLengthSqBefore"] == float(np.float64(p[1, 0] - np.float64(p[0, 0])) ** 2) and st["minLengthSqAfter"] > 0.5
    assert src.tolist() == [0] + list(range(2, 18))
    middle = ((p[0].astype(np.float64) + p[1].astype(np.float64)) * 0.5).astype(np.float32)
    assert v[0].tobytes() == middle.tobytes() and v[1:].tobytes() == p[2:].tobytes()
    assert st["minQualityBefore"] < 0.02 and st["minQualityAfter"] > 0.8
    assert cc.invariants(len(v), t) == cc.invariants(len(p), tri)


def test_rim_vertex_survives_with_its_bits():
    p, tri = cc.disk(rim=True)
    v, t, st, src = cc.collapse(p, tri, MAX_ROUNDS, 0.05)
    assert counts(st, "fixedVertices", "shortBefore", "collapses", "outVertices", "outTriangles") == (9, 1, 1, 9, 7)
    assert src.tolist() == list(range(1, 10)) and v.tobytes() == p[1:].tobytes()      # vertex 0 went, vertex 1 did not move
    assert cc.invariants(len(v), t) == cc.invariants(len(p), tri)


def test_blocked_edges():
    st = cc.collapse(*fc.kite(), MAX_ROUNDS, 10.0)[2]              # both ends fixed: guard (i)
    assert counts(st, "interiorEdges", "fixedVertices", "shortBefore", "blockedAfter", "collapses", "rounds", "converged") == (1, 4, 1, 1, 0, 1, 1)
    st = cc.collapse(*fc.tetrahedron(), MAX_ROUNDS, 100.0)[2]      # closed: nothing fixed, guards (iii) and (iv)
    assert counts(st, "interiorEdges", "fixedVertices", "shortBefore", "blockedAfter", "collapses") == (6, 0, 6, 6, 0)
    p, tri = cc.tube()                                              # a ring of three: guard (iii)
    assert abs(np.linalg.norm(p[1] - p[0]) - 0.017) < 1e-6 and p[3, 2] - p[0, 2] == 1.0
    st = cc.collapse(p, tri, MAX_ROUNDS, 0.05)[2]
    assert counts(st, "fixedVertices", "shortBefore", "blockedAfter", "collapses", "converged") == (6, 12, 12, 0, 1)
    for min_cos in (0.5, 0.0):                                      # the triangle would turn over: guard (v)
        st = cc.collapse(*cc.star(), MAX_ROUNDS, 0.012, min_cos)[2]
        assert counts(st, "shortBefore", "blockedAfter", "collapses") == (1, 1, 0)
    p, tri = cc.star()
    p[4] = cc.disk()[0][4]                                          # without the pulled vertex it is the disk, and collapses
    assert cc.collapse(p, tri, MAX_ROUNDS, 0.012)[2]["collapses"] == 1


def test_coincident_pair_at_length_zero():
    p, tri = cc.coincident()
    v, t, st, _ = cc.collapse(p, tri, MAX_ROUNDS, 0.0)
    assert counts(st, "shortBefore", "collapses", "shortAfter") == (1, 1, 0) and st["minLengthSqBefore"] == 0.0 and st["minQualityBefore"] == 0.0
    assert v[0].tobytes() == p[0].tobytes() and len(t) == len(tri) - 2
    assert cc.collapse(*cc.disk(), MAX_ROUNDS, 0.0)[2]["shortBefore"] == 0


def test_a_row_of_needles_takes_many_rounds():
    p, tri = cc.needle_row()
    trace = []
    v, t, st, _ = cc.collapse(p, tri, MAX_ROUNDS, 0.05, trace=trace)
    assert st["converged"] == 1 and st["rounds"] > 8 and st["shortBefore"] == 19 and st["shortAfter"] == 0
    assert all(r["winners"] >= 1 for r in trace[:-1]) and trace[-1]["candidates"] == 0
    assert cc.invariants(len(v), t) == cc.invariants(len(p), tri)
    st = cc.collapse(p, tri, 3, 0.05)[2]
    assert counts(st, "rounds", "converged") == (3, 0) and st["shortAfter"] > 0
    st = cc.collapse(p, tri, 0, 0.05)[2]                            # a pure report
    assert counts(st, "rounds", "converged", "collapses", "shortBefore", "shortAfter") == (0, 0, 0, 19, 19)


def test_valence_cap_blocks_a_hub():
    p, tri = nc.fan_mesh(100, seed=1)
    st = cc.collapse(p, tri, MAX_ROUNDS, 10.0)[2]
    assert counts(st, "interiorEdges", "shortBefore", "blockedAfter", "collapses", "rounds") == (100, 100, 100, 0, 1)
    for ring, valence, collapses in ((124, 64, 1), (128, 66, 0)):  # the pair of disk() has ring / 2 + 2 triangles at each end
        p, tri = cc.disk(ring)
        assert (tri == 0).any(axis=1).sum() == (tri == 1).any(axis=1).sum() == valence
        assert counts(cc.collapse(p, tri, MAX_ROUNDS, 0.02)[2], "shortBefore", "collapses", "blockedAfter") == (1, collapses, 1 - collapses)


# ---------------------------------------------------------------- the planted needles

def test_planted_needles():
    """64 needles in a 40 x 40 grid: the smallest q goes from below 1e-3 to above 0.2 in two rounds, the second of which
    finds no candidate (this oracle gives 3.97e-6 and 0.294)."""
    p, tri = cc.planted_needles()
    v, t, st, _ = cc.collapse(p, tri, MAX_ROUNDS, 0.05)
    assert counts(st, "collapses", "rounds", "converged", "shortAfter") == (64, 2, 1, 0)
    assert st["minQualityBefore"] < 1e-3 and st["minQualityAfter"] > 0.2
    assert cc.invariants(len(v), t) == cc.invariants(len(p), tri)


# ---------------------------------------------------------------- properties

MESHES = {
    "grid": lambda: (*fc.grid_mesh(40, 40, jitter=0.45, seed=2), 0.5),
    "flat": lambda: (*fc.flat_grid(40, 40, 0.45, 1), 0.5),
    "torus": lambda: (*sc.noisy_torus(60, 20, 0.004, 7), 0.03),
    "needles": lambda: (*cc.planted_needles(), 0.05),
}
TABLE = {"grid": (75, 6), "flat": (145, 8), "torus": (54, 5)}


@pytest.fixture(scope="module", params=sorted(MESHES))
def case(request):
    p, tri, length = MESHES[request.param]()
    return request.param, p, tri, length, cc.collapse(p, tri, MAX_ROUNDS, length)


def test_topology_and_fixed_vertices_stay(case):
    name, p, tri, length, (v, t, st, src) = case
    if name in TABLE:
        assert counts(st, "collapses", "rounds") == TABLE[name]
    assert st["converged"] == 1 and st["shortAfter"] == st["blockedAfter"]
    before = cc.invariants(len(p), tri)
    assert before["manifold"] == 1 and cc.invariants(len(v), t) == before
    # the boundary vertices are fixed: all of them are in the output, in order, with their bits
    sides = set(map(tuple, np.stack([tri.ravel(), tri[:, [1, 2, 0]].ravel()], axis=1).tolist()))
    fixed = sorted(set(x for a, b in sides if (b, a) not in sides for x in (a, b)))
    assert len(fixed) == st["fixedVertices"] and np.isin(fixed, src).all()
    assert v[np.searchsorted(src, fixed)].tobytes() == p[fixed].tobytes()
    assert (np.diff(src.astype(np.int64)) > 0).all() and st["outVertices"] == len(p) - st["collapses"]
    assert st["outTriangles"] == len(tri) - 2 * st["collapses"] and st["unusedVertices"] == st["collapses"]
    moved = np.linalg.norm(v.astype(np.float64) - p[src].astype(np.float64), axis=1)
    assert moved.max() <= length * (1 + 1e-6)       # a midpoint lies half an edge away; a chain of collapses adds up to less than this


def test_again_makes_no_collapse(case):
    _, p, tri, length, (v, t, st, src) = case
    again = cc.collapse(v, t, MAX_ROUNDS, length)
    assert counts(again[2], "collapses", "rounds", "converged", "shortBefore") == (0, 1, 1, st["shortAfter"])
    assert again[0].tobytes() == v.tobytes() and again[1].tolist() == t.tolist()


def test_nothing_short_comes_back_bit_for_bit(case):
    _, p, tri, length, _ = case
    v, t, st, src = cc.collapse(p, tri, MAX_ROUNDS, 0.0)
    assert st["shortBefore"] == 0 and v.tobytes() == p.tobytes() and t.tolist() == tri.tolist() and src.tolist() == list(range(len(p)))


def test_triangle_order_and_corner_rotation(case):
    _, p, tri, length, want = case
    order = np.random.default_rng(3).permutation(len(tri))
    got = cc.collapse(p, tri[order], MAX_ROUNDS, length)
    assert got[2] == want[2] and got[0].tobytes() == want[0].tobytes() and got[3].tolist() == want[3].tolist()
    assert cc.triangle_set(got[1]).tolist() == cc.triangle_set(want[1]).tolist()
    turns = np.random.default_rng(4).integers(0, 3, len(tri))
    turned = np.stack([tri[np.arange(len(tri)), (turns + k) % 3] for k in range(3)], axis=1)
    got = cc.collapse(p, turned, MAX_ROUNDS, length)
    assert got[0].tobytes() == want[0].tobytes() and got[3].tolist() == want[3].tolist()
    assert cc.triangle_set(got[1]).tolist() == cc.triangle_set(want[1]).tolist()
    quality = ("minQualityBefore", "minQualityAfter", "qualityBefore", "qualityAfter")        # q is taken in row order
    assert dict(got[2], **dict((k, want[2][k]) for k in quality)) == want[2]


def test_power_of_two_scaling(case):
    _, p, tri, length, (v, t, st, src) = case
    for shift in (-7, 40):
        s = np.float32(2.0) ** np.float32(shift)
        got = cc.collapse(p * s, tri, MAX_ROUNDS, length * float(s))
        want = dict(st, minLengthSqBefore=st["minLengthSqBefore"] * float(s) ** 2, minLengthSqAfter=st["minLengthSqAfter"] * float(s) ** 2)
        cc.assert_same(got, (v * s, t, want, src))


def test_renumbering_a_tie_free_input():
    p, tri = fc.flat_grid(40, 40, 0.45, 1)
    trace = []
    want = cc.collapse(p, tri, MAX_ROUNDS, 0.5, trace=trace)
    assert not any(r["ties"] for r in trace)
    q, qtri, perm = cc.renumbered(p, tri, 5)
    got = cc.collapse(q, qtri, MAX_ROUNDS, 0.5)
    quality = ("minQualityBefore", "minQualityAfter", "qualityBefore", "qualityAfter")
    assert dict(got[2], **dict((k, want[2][k]) for k in quality)) == want[2]
    assert sorted(map(bytes, got[0].view("V12").ravel())) == sorted(map(bytes, want[0].view("V12").ravel()))


def test_defects_and_unused_vertices_are_dropped():
    p, tri = cc.defect_mesh()
    v, t, st, src = cc.collapse(p, tri, MAX_ROUNDS, 0.6)
    assert counts(st, "outOfRangeTriangles", "degenerateTriangles") == (2, 2) and st["collapses"] > 3
    assert st["unusedVertices"] == 2 + st["collapses"] and len(t) == len(tri) - 4 - 2 * st["collapses"]
    assert not np.isin([len(p) - 2, len(p) - 1], src).any() and t.max() == len(v) - 1
    with pytest.raises(cc.Invalid, match="parameters"):
        cc.collapse(p, tri, 1, -1.0)
    with pytest.raises(cc.Invalid, match="parameters"):
        cc.collapse(p, tri, 1, 0.5, 1.5)


# ---------------------------------------------------------------- the inputs of the GPU tests

def test_gpu_inputs_converge():
    for p, tri, length in ((*fc.grid_mesh(40, 40, jitter=0.45, seed=2), 0.7), (*sc.noisy_torus(200, 40, 0.004, 7), 0.01),
                           (*fc.grid_mesh(300, 300, jitter=0.3, seed=11), 0.5), (*nc.fan_mesh(20_000, seed=1), 10.0),
                           (*cc.defect_mesh(), 0.6), (*fc.flat_grid(9, 11, 0.45, 3), 0.5)):
        st = cc.collapse(p, tri, MAX_ROUNDS, length)[2]
        assert st["converged"] == 1 and st["rounds"] < MAX_ROUNDS
    for build in (cc.disk, fc.kite, fc.tetrahedron, fc.pillow, cc.tube, cc.star, cc.coincident):
        for length, min_cos in ((0.05, 0.5), (100.0, 0.0), (100.0, 1.0)):
            assert cc.collapse(*build(), MAX_ROUNDS, length, min_cos)[2]["converged"] == 1
