"""The CPU oracle of the Delaunay edge flips (flip_cases.py): hand cases with their rows written out, the oracle against a plain
per-triangle restatement of the contract, what the flips achieve on grids, and what the GPU tests rely on -- that their inputs
converge within the rounds they pass, and that the inputs they call free of ties are."""
import math

import numpy as np
import pytest

import flip_cases as fc
import normals_cases as nc
import smooth_cases as sc
import topology_cases as tc

MAX_ROUNDS = 64


# ---------------------------------------------------------------- hand cases

def test_kite_flips():
    p, tri = fc.kite()
    out, st = fc.flip(p, tri, MAX_ROUNDS)
    assert out.tolist() == [[0, 3, 2], [1, 2, 3]]
    assert (st["numEdges"], st["interiorEdges"], st["rounds"], st["flips"], st["converged"]) == (5, 1, 2, 1, 1)
    assert (st["nonDelaunayBefore"], st["nonDelaunayAfter"], st["blockedAfter"]) == (1, 0, 0)
    assert st["minQualityAfter"] > st["minQualityBefore"] > 0 and sum(st["qualityBefore"]) == sum(st["qualityAfter"]) == 2
    out, st = fc.flip(p, tri, 1)                                # the cap on the rounds: flipped, not known to have converged
    assert out.tolist() == [[0, 3, 2], [1, 2, 3]] and (st["rounds"], st["flips"], st["converged"], st["nonDelaunayAfter"]) == (1, 1, 0, 0)
    out, st = fc.flip(p, tri, 0)                                # a pure report
    assert out.tolist() == tri.tolist() and (st["rounds"], st["flips"], st["converged"]) == (0, 0, 0)
    assert (st["nonDelaunayBefore"], st["nonDelaunayAfter"], st["blockedAfter"]) == (1, 1, 0)
    assert (st["minQualityBefore"], st["qualityBefore"]) == (st["minQualityAfter"], st["qualityAfter"])
    out, st = fc.flip(p, tri[:, [1, 2, 0]], MAX_ROUNDS)        # the corners rotated: the same rows
    assert out.tolist() == [[0, 3, 2], [1, 2, 3]]


def test_cocircular_square_stays():
    p, tri = fc.square()
    _, (a, b, c, d, P, _, _) = fc.classify(p.astype(np.float64), tri, np.ones(2, bool), -1.0, fc.MIN_COS)
    assert (a.tolist(), b.tolist(), c.tolist(), d.tolist(), P.tolist()) == ([0], [1], [2], [3], [0.0])
    for min_gain in (0.0, fc.MIN_GAIN):
        out, st = fc.flip(p, tri, MAX_ROUNDS, min_gain)
        assert out.tolist() == tri.tolist() and (st["rounds"], st["flips"], st["converged"], st["nonDelaunayBefore"]) == (1, 0, 1, 0)
        assert st["qualityBefore"] == [0] * 13 + [2, 0, 0]     # 2 sqrt 3 / 4 = 0.866


def test_closed_tetrahedron_is_blocked():
    p, tri = fc.tetrahedron()
    out, st = fc.flip(p, tri, MAX_ROUNDS, min_cos=-1.0)
    assert out.tolist() == tri.tolist() and (st["numEdges"], st["interiorEdges"], st["rounds"], st["converged"]) == (6, 6, 1, 1)
    assert st["nonDelaunayBefore"] == st["nonDelaunayAfter"] == st["blockedAfter"] >= 1


def test_pillow_has_no_interior_regular_edge():
    p, tri = fc.pillow()
    out, st = fc.flip(p, tri, MAX_ROUNDS)
    assert out.tolist() == tri.tolist() and (st["numEdges"], st["interiorEdges"], st["nonDelaunayBefore"]) == (3, 0, 0)


def test_fold_and_dart():
    p, tri = fc.folded()
    out, st = fc.flip(p, tri, MAX_ROUNDS, min_cos=0.5)          # guard (ii)
    assert out.tolist() == tri.tolist() and (st["nonDelaunayBefore"], st["blockedAfter"], st["flips"]) == (1, 1, 0)
    out, st = fc.flip(p, tri, MAX_ROUNDS, min_cos=-1.0)         # (ii) lets it pass, and (iii) finds the quad convex
    assert out.tolist() == [[0, 3, 2], [1, 2, 3]] and (st["flips"], st["blockedAfter"]) == (1, 0)
    p, tri = fc.concave()
    for min_cos in (0.5, -1.0):                                 # at -1 guard (ii) holds with equality: (iii) blocks
        out, st = fc.flip(p, tri, MAX_ROUNDS, min_cos=min_cos)
        assert out.tolist() == tri.tolist() and (st["nonDelaunayBefore"], st["blockedAfter"], st["flips"]) == (1, 1, 0)


def test_zero_area_cap_flips():
    p, tri = fc.cap()
    _, (_, _, _, _, P, _, _) = fc.classify(p.astype(np.float64), tri, np.ones(2, bool), fc.MIN_GAIN, fc.MIN_COS)
    assert P.tolist() == [math.inf]
    out, st = fc.flip(p, tri, MAX_ROUNDS)
    assert out.tolist() == [[0, 3, 2], [1, 2, 3]] and (st["flips"], st["converged"]) == (1, 1)
    assert st["minQualityBefore"] == 0.0 and st["qualityBefore"][0] == 1 and st["minQualityAfter"] > 0.5


def test_parameters_and_vertices_are_checked():
    p, tri = fc.kite()
    for min_gain, min_cos in [(-1e-9, 0.5), (math.inf, 0.5), (math.nan, 0.5), (0.0, 1.5), (0.0, -1.5), (0.0, math.nan)]:
        with pytest.raises(fc.Invalid, match="parameters"):
            fc.flip(p, tri, 1, min_gain, min_cos)
    p[2, 1] = np.nan
    with pytest.raises(fc.Invalid, match="vertex"):
        fc.flip(p, tri, 1)


# ---------------------------------------------------------------- a plain restatement

def plain_flip(vertices, triangles, max_rounds, min_gain, min_cos):
    """The contract in include/mlsgpu_hip.h read aloud: Python floats (doubles), a dict of directed sides, loops."""
    P3 = [tuple(float(x) for x in row) for row in np.asarray(vertices, np.float32)]
    tri = [[int(x) for x in row] for row in triangles]
    V = len(P3)

    def sub(u, v): return (u[0] - v[0], u[1] - v[1], u[2] - v[2])
    def dot(u, v): return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    def cross(u, v): return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    def face(p, q, r): return cross(sub(q, p), sub(r, p))

    def div(x, y):
        if y != 0:
            return x / y
        return math.nan if x == 0 or x != x else math.copysign(math.inf, x)

    def cot(p, q, r):
        x = cross(sub(q, p), sub(r, p))
        return div(dot(sub(q, p), sub(r, p)), math.sqrt(dot(x, x)))

    live = [all(i < V for i in t) and len(set(t)) == 3 for t in tri]

    def quality():
        least, hist = math.inf, [0] * 16
        for t, row in enumerate(tri):
            if live[t]:
                p, q, r = (P3[i] for i in row)
                x, u, v, w = face(p, q, r), sub(q, p), sub(r, q), sub(p, r)
                den = (dot(u, u) + dot(v, v)) + dot(w, w)
                value = div(fc.TWO_ROOT_THREE * math.sqrt(dot(x, x)), den)
                if den == 0 or value != value:
                    value = 0.0
                least = min(least, value)
                hist[min(15, math.floor(16 * value))] += 1
        return (least if least != math.inf else 0.0), hist

    st = fc.empty_stats()
    st.update(numVertices=V, numTriangles=len(tri), outOfRangeTriangles=sum(any(i >= V for i in t) for t in tri))
    st["degenerateTriangles"] = len(tri) - sum(live) - st["outOfRangeTriangles"]
    st["minQualityBefore"], st["qualityBefore"] = quality()
    first = True
    while True:
        sides = {}
        for t, row in enumerate(tri):
            if live[t]:
                for k in range(3):
                    sides.setdefault((row[k], row[(k + 1) % 3]), []).append((t, row[(k + 2) % 3]))
        interior, bad, blocked, cands = 0, 0, 0, []
        for (a, b), users in sides.items():
            back = sides.get((b, a), [])
            if not (a < b and len(users) == 1 and len(back) == 1):
                continue
            (t1, c), (t2, d) = users[0], back[0]
            if c == d:
                continue
            interior += 1
            pa, pb, pc, pd = P3[a], P3[b], P3[c], P3[d]
            P = -(cot(pc, pa, pb) + cot(pd, pb, pa))
            if not P > min_gain:
                continue
            bad += 1
            n1, n2, m1, m2 = face(pa, pb, pc), face(pb, pa, pd), face(pa, pd, pc), face(pb, pc, pd)
            N = (n1[0] + n2[0], n1[1] + n2[1], n1[2] + n2[2])
            if ((c, d) in sides or (d, c) in sides or not dot(n1, n2) >= (min_cos * math.sqrt(dot(n1, n1))) * math.sqrt(dot(n2, n2))
                    or not (dot(m1, N) > 0 and dot(m2, N) > 0)):
                blocked += 1
                continue
            cands.append((-P, a, b, c, d, t1, t2))              # sorted: the larger P first, then the smaller (a, b)
        if first:
            st.update(numEdges=len(set((min(s), max(s)) for s in sides)), interiorEdges=interior, nonDelaunayBefore=bad)
            first = False
        st.update(nonDelaunayAfter=bad, blockedAfter=blocked)
        if st["rounds"] == max_rounds:
            break
        st["rounds"] += 1
        if not cands:
            st["converged"] = 1
            break
        cands.sort()
        for me in cands:                                        # wins if no better candidate shares a vertex
            if not any(other < me and set(other[1:5]) & set(me[1:5]) for other in cands):
                _, a, b, c, d, t1, t2 = me
                tri[t1], tri[t2] = [a, d, c], [b, c, d]
                st["flips"] += 1
    st["minQualityAfter"], st["qualityAfter"] = quality()
    return np.array(tri, np.uint32).reshape(-1, 3), st


@pytest.mark.parametrize("mesh", ["flat", "bumpy", "defects", "hands"])
def test_oracle_against_the_plain_restatement(mesh):
    if mesh == "hands":
        for build in (fc.kite, fc.square, fc.tetrahedron, fc.pillow, fc.folded, fc.concave, fc.cap):
            for min_cos in (0.5, -1.0):
                fc.assert_same(fc.flip(*build(), MAX_ROUNDS, 0.0, min_cos), plain_flip(*build(), MAX_ROUNDS, 0.0, min_cos))
        return
    p, tri = {"flat": lambda: fc.flat_grid(12, 12, 0.3, 5), "bumpy": lambda: fc.grid_mesh(12, 12, jitter=0.45, seed=6),
              "defects": fc.defect_mesh}[mesh]()
    for rounds in (0, 1, 2, MAX_ROUNDS):
        want = plain_flip(p, tri, rounds, fc.MIN_GAIN, fc.MIN_COS)
        fc.assert_same(fc.flip(p, tri, rounds), want)
    assert want[1]["flips"] > 5 and want[1]["converged"] == 1


# ---------------------------------------------------------------- what the flips achieve

def invariants(p, tri, out):
    """The edge count and the Euler characteristic stay (the edges themselves change)."""
    assert len(fc.edge_set(out, len(p))) == len(fc.edge_set(tri, len(p)))
    before, after = tc.count_all(len(p), np.asarray(tri)), tc.count_all(len(p), out.astype(np.int64))
    for name in ("eulerCharacteristic", "edges", "boundaryEdges", "numComponents", "numBoundaries", "manifold"):
        assert before[name] == after[name], name


def test_flat_jittered_grid_becomes_delaunay():
    p, tri = fc.flat_grid(40, 40, 0.3, 1)
    trace = []
    out, st = fc.flip(p, tri, MAX_ROUNDS, trace=trace)
    assert st["converged"] == 1 and st["nonDelaunayAfter"] == 0 and st["rounds"] < 20 and st["flips"] > 300
    assert st["minQualityAfter"] > st["minQualityBefore"]
    low = [k for k in range(4) if st["qualityBefore"][k] > 0 and st["qualityAfter"][k] == 0]
    assert low, (st["qualityBefore"], st["qualityAfter"])
    assert sum(st["qualityBefore"]) == sum(st["qualityAfter"]) == len(tri)
    assert [r["winners"] for r in trace][-1] == 0 and all(0 < r["winners"] <= r["candidates"] for r in trace[:-1])
    invariants(p, tri, out)
    again, st2 = fc.flip(p, out, MAX_ROUNDS)                    # a fixed point
    assert again.tolist() == out.tolist() and (st2["rounds"], st2["flips"], st2["nonDelaunayBefore"]) == (1, 0, 0)


def test_bumpy_grid_keeps_what_the_guards_refuse():
    p, tri = fc.grid_mesh(40, 40, jitter=0.45, seed=2)
    out, st = fc.flip(p, tri, MAX_ROUNDS)
    assert st["converged"] == 1 and st["nonDelaunayAfter"] == st["blockedAfter"] > 0 and st["flips"] > 100
    invariants(p, tri, out)


# ---------------------------------------------------------------- what the GPU tests rely on

def gpu_inputs():
    """name -> (vertices, triangles, maxRounds, free of ties): every mesh test_gpu_flip.py runs to convergence."""
    big = fc.grid_mesh(300, 300, jitter=0.3, seed=11)
    return {"flat40": fc.flat_grid(40, 40, 0.3, 1) + (MAX_ROUNDS, True), "bumpy40": fc.grid_mesh(40, 40, jitter=0.45, seed=2) + (MAX_ROUNDS, True),
            "big": big + (MAX_ROUNDS, False), "big-1": (big[0], big[1][:-1], MAX_ROUNDS, False),
            "torus": sc.noisy_torus(200, 40, 0.004, 7) + (MAX_ROUNDS, False), "defects": fc.defect_mesh() + (MAX_ROUNDS, False), "small": fc.flat_grid(9, 11, 0.3, 3) + (MAX_ROUNDS, False)}


def test_gpu_inputs_converge_and_have_no_ties():
    for name, (p, tri, rounds, no_ties) in gpu_inputs().items():
        trace = []
        _, st = fc.flip(p, tri, rounds, trace=trace)
        assert st["converged"] == 1 and st["rounds"] < rounds and st["flips"] > 0, (name, st)
        if no_ties:
            assert not any(r["ties"] for r in trace), name
    p, tri = nc.fan_mesh(20_000, seed=1)                        # run for 3 rounds only: thousands of candidates on one hub
    trace = []
    fc.flip(p, tri, 3, trace=trace)
    assert trace[0]["candidates"] > 2000 and [r["winners"] for r in trace] == [1, 1, 1], trace
