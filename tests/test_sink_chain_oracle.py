"""The inputs and parameters of sink_chain_cases.py have the properties that tests/test_gpu_sink_chain.py rests on, shown with the
numpy model alone (the sink's chunks taken from mesher_oracle.mesh_sink), so that a pass on the GPU cannot be vacuous.  Runs
without a GPU.

Parameters settled on, all as first proposed: 64 rounds, fill_holes(32), split_edges(0.8), collapse_edges(0.45), smooth(3),
simplify cell 2.5 and quadric cell 5.0 from origin (-22.5, -2.5, -5.0) -- at this origin the simplified tiles have stray
coincidences between chunks, so it did not have to move --, and the cell that empties everything: 64 from (-24, -4, -8).
The sheet is shifted by -20 in x, which puts grid column 20 at x = 0 for the -0.0 / +0.0 pair of `twins`."""
import time

import numpy as np
import pytest

import repair_cases as rc
import sink_chain_cases as k
from sink_cases import mo

SPENT = [0.0]          # seconds in the tests of this file so far


@pytest.fixture(autouse=True)
def spent():
    start = time.perf_counter()
    yield
    SPENT[0] += time.perf_counter() - start


def model_of(name):
    meshes, prune = k.variant(name)
    out, stats = mo.mesh_sink(meshes, prune)
    return k.SinkModel.from_output(out, k.quiet_chunks(meshes, prune)), stats


def holders(model):
    """Per distinct position of the dense chunks: how many chunks hold it."""
    rows = np.concatenate([k.rows12(d[1]) for d in model.dense])
    chunk = np.repeat(np.arange(len(model.dense)), [len(d[1]) for d in model.dense])
    _, row_id = np.unique(rows, axis=0, return_inverse=True)
    pairs = np.unique(row_id.reshape(-1) * len(model.dense) + chunk)
    return np.bincount(pairs // len(model.dense))


@pytest.mark.parametrize("name,chain", [("tiles", "S1"), ("gaps", "S1"), ("twins", "S1"), ("tiles", "S2"), ("crumb", "S2"), ("tiles", "S3")])
def test_chains_converge_and_keep_the_seams_closed(name, chain):
    """Every split, collapse and flip of the chains converges within 64 rounds on every chunk, and up to the last step before a
    simplify every seam is closed in the model -- what the GPU test then asserts of the device."""
    model, _ = model_of(name)
    simplified = False
    assert k.open_seams(model.chunks()) == []
    for step, args, _ in getattr(k, chain):
        getattr(model, step)(*args)
        simplified = simplified or step.startswith("simplify")
        if not simplified:
            assert k.open_seams(model.chunks()) == [], step
    assert all(converged == 1 and rounds <= k.MAX_ROUNDS for _, _, rounds, converged in model.rounds), model.rounds
    if chain != "S3":
        assert {stage for stage, _, _, _ in model.rounds} == {"split", "collapse", "flip"}
        assert max(rounds for _, _, rounds, _ in model.rounds) > 5


def test_tiles_positions_held_by_two_and_by_four_chunks():
    model, stats = model_of("tiles")
    count = holders(model)
    assert set(count) == {1, 2, 4} and (count == 4).sum() == 4 and (count == 2).sum() == 4 * 49 - 2 * 4
    assert sorted(int(m.sum()) for m in model.masks()) == [33] * 4 + [49] * 4 + [64]
    assert stats["components"] == 1 and [len(t) for _, _, t in model.chunks()] == [510, 510, 510, 512, 510, 512, 510, 512, 510]


def test_twins_pin_what_the_rule_says():
    meshes, where = k.twins()
    plain, _ = model_of("tiles")
    model, _ = model_of("twins")
    pinned, before = model.masks(), plain.masks()
    P = k.sheet()

    def at(tile, position):
        return np.flatnonzero((k.rows12(model.dense[tile][1]) == k.rows12(position)).all(axis=1))

    # (a) tile 4 holds the seam position twice and tile 3 once: all three are pinned
    mine, theirs = at(4, P[k.TWIN_SEAM]), at(3, P[k.TWIN_SEAM])
    assert len(mine) == 2 and len(theirs) == 1 and pinned[4][mine].all() and pinned[3][theirs].all()
    assert [int(m.sum()) for m in pinned] == [int(m.sum()) + (t == 4) for t, m in enumerate(before)]
    # (b) tile 7 holds a position twice that nobody else has: nothing is pinned
    both = at(7, P[k.TWIN_INNER])
    assert len(both) == 2 and not pinned[7][both].any() and all(len(at(t, P[k.TWIN_INNER])) == 0 for t in range(9) if t != 7)
    # (c) -0.0 in tile 1 against +0.0 in tile 0: equal as floats, other bytes, nothing is pinned
    minus, plus = P[k.ZERO_AT].copy(), P[k.ZERO_AT].copy()
    plus[0] = np.float32(0.0)
    assert np.signbit(minus[0]) and minus[0] == plus[0] and not np.array_equal(k.rows12(minus), k.rows12(plus))
    a, b = at(1, minus), at(0, plus)
    assert len(a) == 1 and len(b) == 1 and not pinned[1][a].any() and not pinned[0][b].any()
    assert len(at(0, minus)) == 0 and len(at(1, plus)) == 0
    for name in "abc":                                              # the new vertices are where twins() says
        tile, index = where[name]
        assert meshes[tile]["vertices"][index].tobytes() == {"a": P[k.TWIN_SEAM], "b": P[k.TWIN_INNER], "c": plus}[name].tobytes()
    st = model.fill_holes(k.FILL_EDGES)                             # the fans' loops: (a) stays open, (b) and (c) are capped
    assert (st["pinnedLoops"], st["filledLoops"]) == (1, plain.fill_holes(k.FILL_EDGES)["filledLoops"] + 2)


def test_gaps_drops_the_island_and_keeps_every_tile_whole():
    meshes, prune = k.variant("gaps")
    everything, stats0 = mo.mesh_sink(meshes, 0.0)
    out, stats = mo.mesh_sink(meshes, prune)
    assert stats0["components"] == 2 and stats["kept_components"] == 1 and stats["threshold"] == 6
    assert [c for c, _, _ in everything] == [k.GAP_IDS[0], k.GAP_IDS[1], k.GAP_IDS[2], k.ISLAND_ID] + list(k.GAP_IDS[3:])
    assert [c for c, _, _ in out] == list(k.GAP_IDS)                # the island's chunk is gone, nothing else
    whole = mo.mesh_sink(k.tiles())[0]
    assert [(len(v), len(t)) for _, v, t in out] == [(len(v), len(t)) for _, v, t in whole]
    for (_, v, t), (_, wv, wt) in zip(out, whole):
        assert mo.isomorphic(v, t, wv, wt)
    model, _ = model_of("gaps")
    assert len(model.dense) == 11 and model.out == [0, 2, 3, 5, 6, 7, 8, 9, 10]            # dense and output numbers differ
    assert [d[0] for d in model.dense][1::3][:2] == [k.QUIET_ID, k.ISLAND_ID]
    assert (len(model.dense[1][1]), len(model.dense[1][2]), len(model.dense[4][1])) == (4, 0, 0)
    ids = [m["chunk"] for m in meshes]
    assert ids != sorted(ids) and len(set(ids)) == 11 and max(ids) > 2 ** 24               # neither dense nor monotonic
    assert any(ids.index(c) < i for i, c in enumerate(ids) if i > 0 and ids[i - 1] != c)  # blocks of the chunks interleave
    pinned = model.masks()
    assert pinned[1].all() and int(pinned[6].sum()) == 64 + 4      # the chunk without output pins tile 4's copies of its vertices
    assert model.fill_holes(k.FILL_EDGES)["pinnedLoops"] == 1 and len(model.dense[1][1]) == 0
    assert int(model.masks()[6].sum()) == 64                       # a new generation keeps nothing of a chunk without triangles


def test_crumb_is_swallowed_whole():
    model, _ = model_of("crumb")
    assert len(model.dense[9][2]) == 8
    model.simplify(k.SIMPLIFY_ORIGIN, k.SIMPLIFY_CELL)
    assert [len(d[2]) for d in model.dense][9] == 0 and len(model.dense[9][1]) == 0 and model.out[-1] == 9
    assert all(len(d[2]) > 50 for d in model.dense[:9])


def test_simplified_tiles_have_open_seams_stray_coincidences_and_twins_after_repair():
    model, _ = model_of("tiles")
    model.simplify(k.SIMPLIFY_ORIGIN, k.SIMPLIFY_CELL)
    shared = int((holders(model) > 1).sum())                        # 192 positions before; the clusters of two chunks differ
    strays = sum(int(m.sum()) for m in model.masks())
    print("positions shared after simplify:", shared, "pinned vertices:", strays)
    assert 0 < shared < 192 // 4 and strays >= 2 * shared           # the seams are open, yet the mask is not all zero
    model.repair(0)
    st = model.repair(rc.SPLIT_PINCHES)
    assert st["splitVertices"] > 0
    assert any(len(np.unique(k.rows12(d[1]), axis=0)) < len(d[1]) for d in model.dense)


def test_everything_emptied():
    model, _ = model_of("tiles")
    model.simplify(k.EMPTY_ORIGIN, k.EMPTY_CELL)
    assert all(len(d[1]) == 0 and len(d[2]) == 0 for d in model.dense) and len(model.out) == 9
    st = model.flip_edges(k.MAX_ROUNDS)
    assert (st["converged"], st["rounds"], st["numTriangles"]) == (1, 0, 0)
    assert model.collapse_edges(k.MAX_ROUNDS, k.COLLAPSE_LENGTH)["minLengthSqBefore"] == np.inf
    assert model.finalize() == 9 and sum(len(d[2]) for d in model.dense) == 2 * (48 * 48 - len(k.HOLES))


def test_the_file_runs_in_under_a_minute():
    """Collected last: every test above has added its time."""
    assert 1 < SPENT[0] < 60
