"""The self-intersection oracle (intersect_cases.self_intersections) against answers known by hand, and its two routes --
brute force and the grid -- against each other."""
import numpy as np
import pytest

import fill_cases as fc
import intersect_cases as ic


@pytest.mark.parametrize("case", ic.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, v, t, crossing = case
    for prune in (False, True):
        partners, pairs, st = ic.self_intersections(v, t, prune=prune)
        assert st["crossingPairs"] == crossing and st["candidatePairs"] == 1, name
        assert pairs.tolist() == ([[0, 1]] if crossing else []) and partners.tolist() == [crossing, crossing]
        assert (st["lowestA"], st["lowestB"]) == ((0, 1) if crossing else (ic.NONE, ic.NONE))
        assert (st["maxPartners"], st["maxPartnersTriangle"]) == ((1, 0) if crossing else (0, ic.NONE))
        assert st["crossingTriangles"] == 2 * crossing
    # the answer does not hang on which triangle comes first
    assert ic.self_intersections(v, t[::-1])[2]["crossingPairs"] == crossing


def test_zero_rows_are_exactly_zero():
    """A point equal to a corner gives det == perm * 0 == 0 whatever the other coordinates are."""
    rng = np.random.default_rng(1)
    a, b, c = (tuple(rng.normal(size=(3, 1000)) * 1e3) for _ in range(3))
    for x in (a, b, c):
        assert not ic.orient(a, b, c, x).any()
    assert (ic.orient(a, b, c, tuple(rng.normal(size=(3, 1000)))) != 0).sum() > 990


def jittered():
    return fc.grid_mesh(40, 40, jitter=0.3, seed=3)


def flat():
    p, tri = jittered()
    p = p.copy()
    p[:, 2] = 0
    return p, tri


def rotated():
    p, tri = flat()
    a, b = 0.7, 0.4
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    return (p.astype(np.float64) @ (rx @ rz).T).astype(np.float32), tri


def folded(p, tri):
    p = p.copy()
    p[20 * 40 + 20] += np.float32([3.3, 2.7, 0])
    return p, tri


def two_sheets():
    p, tri = jittered()
    q, _ = fc.grid_mesh(40, 40, jitter=0.3, seed=4)
    return ic.joined((p, tri), (ic.tilted(q), tri))


MESHES = [("jittered", jittered, 0, 0), ("flat", flat, 0, 0), ("rotated", rotated, 0, 0),
          ("twice", lambda: ic.joined(jittered(), jittered()), 0, 0), ("folded", lambda: folded(*jittered()), 20, None),
          ("folded_flat", lambda: folded(*flat()), 0, 0), ("two_sheets", two_sheets, 223, 213)]


@pytest.mark.parametrize("mesh", MESHES, ids=lambda m: m[0])
def test_routes_agree(mesh):
    name, make, crossing, triangles = mesh
    v, t = make()
    want = ic.self_intersections(v, t, prune=False)
    ic.assert_same(ic.self_intersections(v, t, prune=True), want)
    st = want[2]
    assert st["crossingPairs"] == crossing and len(want[1]) == crossing
    assert triangles is None or st["crossingTriangles"] == triangles
    assert st["candidatePairs"] >= len(t)               # neighbours are candidates
    assert want[0].sum() == 2 * crossing and (want[0] > 0).sum() == st["crossingTriangles"]
    if name == "twice":
        assert st["candidatePairs"] > 4 * ic.self_intersections(*jittered())[2]["candidatePairs"]


def test_corner_order_on_two_sheets():
    """Rotating or flipping every triangle's corner order leaves the pair list as it is -- on this mesh: the contract does not
    promise it in general."""
    v, t = two_sheets()
    want = ic.self_intersections(v, t)
    for order in ([1, 2, 0], [2, 0, 1], [0, 2, 1], [2, 1, 0]):
        got = ic.self_intersections(v, t[:, order])
        np.testing.assert_array_equal(got[1], want[1])
        assert got[2]["candidatePairs"] == want[2]["candidatePairs"]


def test_defects_and_refusals():
    v, t = two_sheets()
    bad = t.copy()
    bad[5] = [7, 7, 9]
    bad[11, 2] = len(v)
    _, _, st = ic.self_intersections(v, bad)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (1, 1)
    w = v.copy()
    w[3, 1] = np.nan
    with pytest.raises(ic.Invalid):
        ic.self_intersections(w, t)
    none = ic.self_intersections(np.zeros((0, 3), np.float32), t[:4])[2]
    assert none["outOfRangeTriangles"] == 4 and none["lowestA"] == ic.NONE


def test_combined():
    one = ic.self_intersections(*two_sheets())[2]
    clean = ic.self_intersections(*jittered())[2]
    total = ic.combined([clean, one, one])
    assert (total["lowestChunk"], total["crossingChunks"], total["crossingPairs"]) == (1, 2, 446)
    assert (total["lowestA"], total["lowestB"], total["maxPartners"]) == (one["lowestA"], one["lowestB"], one["maxPartners"])
    assert ic.combined([clean])["lowestA"] == ic.NONE
