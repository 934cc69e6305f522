"""The repair contract on the CPU: repair_cases.repair against topology_cases.count_all, hand cases, invariances."""
import numpy as np
import pytest

import repair_cases as rc
import topology_cases as tc

FLAGS = (0, rc.SPLIT_PINCHES)


def identities(stats):
    s = stats
    assert s["outVertices"] == s["numVertices"] - s["unusedVertices"] + s["addedVertices"]
    assert s["outTriangles"] == s["numTriangles"] - s["outOfRangeTriangles"] - s["degenerateTriangles"] - s["droppedTriangles"]
    assert s["splitVertices"] <= s["addedVertices"] and (s["splitVertices"] == 0) == (s["addedVertices"] == 0)
    assert s["droppedTriangles"] <= s["repeatedSides"] and (s["droppedTriangles"] == 0) == (s["repeatedSides"] == 0)
    assert list(s) == list(rc.STAT_NAMES)


def test_random_meshes_become_manifold_and_manifold_ones_stay():
    """3 000 draws: whatever comes in, the topology oracle calls the output manifold under both flags, and what it called
    manifold before comes back unchanged without flags."""
    rng = np.random.default_rng(5)
    before = 0
    for _ in range(3000):
        V, tri = tc.random_mesh(rng)
        p = rc.positions(V, 7)
        was = tc.count_all(V, tri)["manifold"]
        before += not was
        for flags in FLAGS:
            out = rc.repair(p, tri, flags)
            identities(out[2])
            if out[2]["outTriangles"] > 0 or V == 0:
                assert rc.report(out)["count"] == [0] * 6, (V, tri.tolist(), flags)
            else:
                assert len(out[0]) == 0 and len(out[1]) == 0
            np.testing.assert_array_equal(out[0].view(np.uint32), p[out[3]].view(np.uint32))
        if was:
            out = rc.repair(p, tri, 0)
            np.testing.assert_array_equal(out[0].view(np.uint32), p.view(np.uint32))
            np.testing.assert_array_equal(out[1], tri.astype(np.uint32))
            np.testing.assert_array_equal(out[3], np.arange(V))
    assert before > 2000                # most draws are defective: the test would show little otherwise


@pytest.mark.parametrize("spec", rc.TORI)
def test_simplified_tori(spec):
    p, tri = rc.simplified_torus(*spec)
    was = tc.count_all(len(p), tri)
    assert was["manifold"] == 0 and was["count"][tc.DUPLICATED] > 0
    for flags in FLAGS:
        out = rc.repair(p, tri, flags)
        identities(out[2])
        assert rc.report(out)["manifold"] == 1
        assert out[2]["droppedTriangles"] > 0
        rc.assert_same(rc.repair(out[0], out[1], flags), (out[0], out[1], stats_of(len(out[0]), len(out[1])),
                                                         np.arange(len(out[0]))))


def stats_of(V, T, **other):
    s = dict.fromkeys(rc.STAT_NAMES, 0)
    s.update(numVertices=V, numTriangles=T, outVertices=V, outTriangles=T)
    s.update(other)
    return s


def test_bowtie():
    """hub 0 with the rings 1..4 and 5..9: two rings, keys 1 and 5, so the second cone's hub is output vertex 1."""
    p, tri = rc.bowtie(4, 5)
    assert tc.count_all(len(p), tri)["count"][tc.TUNNEL] == 1
    for flags in FLAGS:
        v, t, s, src = rc.repair(p, tri, flags)
        assert src.tolist() == [0, 0] + list(range(1, 10))
        assert t.tolist() == [[0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 2], [1, 6, 7], [1, 7, 8], [1, 8, 9], [1, 9, 10], [1, 10, 6]]
        assert s == stats_of(10, 9, splitVertices=1, addedVertices=1, outVertices=11)


def test_bowtie_with_the_hub_in_the_middle():
    """the hub is vertex 6: the groups of a vertex follow each other in the numbering, the others keep their order"""
    p, tri = rc.bowtie(4, 5, hub=6)
    v, t, s, src = rc.repair(p, tri, 0)
    assert src.tolist() == [0, 1, 2, 3, 4, 5, 6, 6, 7, 8, 9]
    assert t[:4].tolist() == [[6, 0, 1], [6, 1, 2], [6, 2, 3], [6, 3, 0]]          # the ring with key 0
    assert t[4:].tolist() == [[7, 4, 5], [7, 5, 8], [7, 8, 9], [7, 9, 10], [7, 10, 4]]
    assert rc.report((v, t))["manifold"] == 1


def test_cone_and_fan():
    p, tri = rc.cone_and_fan(4, 3)
    assert tc.count_all(len(p), tri)["count"][tc.MIXED] == 1
    for flags in FLAGS:
        v, t, s, src = rc.repair(p, tri, flags)
        assert src.tolist() == [0, 0] + list(range(1, 9))
        assert t.tolist() == [[0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 2], [1, 6, 7], [1, 7, 8], [1, 8, 9]]
        assert s == stats_of(9, 7, splitVertices=1, addedVertices=1, outVertices=10)


def test_cone_and_two_fans():
    """without flags the chains of a mixed vertex stay together; under the flag each gets its own vertex"""
    p = rc.positions(11, 4)
    tri = np.concatenate([rc.fan(2, 0, 1), tc.cone(4, 0, 4), rc.fan(2, 0, 8)])        # chain 1.., ring 4..7, chain 8..
    v, t, s, src = rc.repair(p, tri, 0)
    assert src.tolist()[:2] == [0, 0] and s["splitVertices"] == 1 and s["addedVertices"] == 1
    assert sorted(set(t[:2, 0].tolist() + t[6:, 0].tolist())) == [0] and set(t[2:6, 0].tolist()) == {1}
    v, t, s, src = rc.repair(p, tri, rc.SPLIT_PINCHES)
    assert src.tolist()[:3] == [0, 0, 0] and s["splitVertices"] == 1 and s["addedVertices"] == 2
    assert t[:, 0].tolist() == [0, 0, 1, 1, 1, 1, 2, 2]
    assert rc.report((v, t))["manifold"] == 1


def test_two_fans():
    p, tri = rc.two_fans(2, 3)
    assert tc.count_all(len(p), tri)["manifold"] == 1
    v, t, s, src = rc.repair(p, tri, 0)
    np.testing.assert_array_equal(t, tri)
    np.testing.assert_array_equal(v.view(np.uint32), p.view(np.uint32))
    assert s == stats_of(8, 5)
    v, t, s, src = rc.repair(p, tri, rc.SPLIT_PINCHES)
    assert src.tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7]
    assert t.tolist() == [[0, 2, 3], [0, 3, 4], [1, 5, 6], [1, 6, 7], [1, 7, 8]]
    assert s == stats_of(8, 5, splitVertices=1, addedVertices=1, outVertices=9)


def test_fin_and_twice():
    p, tri = rc.fin(4, 4)
    for flags in FLAGS:
        v, t, s, src = rc.repair(p, tri, flags)
        # the fin and the grid triangle with the same directed side both go; the fin's tip is unused then
        assert s == stats_of(17, 19, repeatedSides=2, droppedTriangles=2, unusedVertices=1, outVertices=16, outTriangles=17)
        assert rc.report((v, t))["manifold"] == 1
    p, tri = rc.twice(3, 4)
    for flags in FLAGS:
        v, t, s, src = rc.repair(p, tri, flags)
        assert s == stats_of(12, 13, repeatedSides=6, droppedTriangles=2, outTriangles=11)
        np.testing.assert_array_equal(t, np.delete(tri[:12], 3, axis=0))


def test_classification_trap():
    """(1, 1, 7) is out of range here, as for smoothing and hole filling, where the topology report calls it degenerate"""
    p, tri = tc.classification_trap()
    v, t, s, src = rc.repair(p, tri, 0)
    assert s == stats_of(4, 5, outOfRangeTriangles=2, degenerateTriangles=1, outTriangles=2)
    np.testing.assert_array_equal(t, tri[:2])


def test_empty_inputs():
    none_v, none_t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    assert rc.repair(none_v, none_t)[2] == stats_of(0, 0)
    assert rc.repair(none_v, [[0, 1, 2]])[2] == stats_of(0, 1, outOfRangeTriangles=1, outTriangles=0)
    assert rc.repair(rc.positions(3), none_t)[2] == stats_of(3, 0, unusedVertices=3, outVertices=0)
    s = rc.repair(rc.positions(3), [[0, 1, 2], [0, 1, 2]])[2]
    assert s == stats_of(3, 2, repeatedSides=6, droppedTriangles=2, unusedVertices=3, outVertices=0, outTriangles=0)
    with pytest.raises(rc.Invalid):
        rc.repair(none_v, none_t, 2)


@pytest.mark.parametrize("flags", FLAGS)
def test_invariance_and_idempotence(flags):
    rng = np.random.default_rng(11)
    meshes = [rc.bowtie(5, 7, hub=3), rc.cone_and_fan(), rc.fin(5, 6), rc.simplified_torus(*rc.TORI[0])]
    for _ in range(200):
        V, tri = tc.random_mesh(rng)
        meshes.append((rc.positions(V, 9), tri))
    for p, tri in meshes:
        v, t, s, src = rc.repair(p, tri, flags)
        # permuting the triangles permutes the output triangles and nothing else
        order = rng.permutation(len(tri))
        pv, pt, ps, psrc = rc.repair(p, tri[order], flags)
        assert ps == s
        np.testing.assert_array_equal(psrc, src)
        kept = np.flatnonzero(kept_mask(p, tri))
        np.testing.assert_array_equal(pt, t[np.searchsorted(kept, order[np.isin(order, kept)])])
        # renumbering the vertices keeps the soup
        perm = rng.permutation(len(p))
        rp = np.empty_like(p)
        rp[perm] = p
        rtri = np.where(tri < len(p), perm[np.minimum(tri, len(p) - 1)], tri)
        rv, rt, rs, _ = rc.repair(rp, rtri, flags)
        assert rs == s
        assert rc.soup(rv, rt) == rc.soup(v, t)
        # repairing twice is repairing once
        again = rc.repair(v, t, flags)
        np.testing.assert_array_equal(again[0].view(np.uint32), v.view(np.uint32))
        np.testing.assert_array_equal(again[1], t)
        assert again[2] == stats_of(len(v), len(t))


def kept_mask(p, tri):
    """The triangles that steps 1 and 2 keep, straight from their definition."""
    V = len(p)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    live = (tri < V).all(axis=1) & (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0])
    sides = {}
    for t in np.flatnonzero(live):
        for j in range(3):
            sides.setdefault((int(tri[t, j]), int(tri[t, (j + 1) % 3])), []).append(t)
    keep = live.copy()
    for users in sides.values():
        if len(users) > 1:
            keep[users] = False
    return keep
