"""entryScatterKernel ranks a tile's entries from a bit matrix (one bit per digit and splat, 64 splats to a word): clouds
at the edges of a word, of a tile and of the argument that lets it (no two entries of a splat share a digit).  Every case
compares `start` and `commands` word for word with the oracle's tree."""
import numpy as np
import pytest

import oracle_binding as ob
import tree_cases as tc
from gpu_common import ctx  # noqa: F401
from test_gpu_tree import build_and_compare

pytestmark = pytest.mark.gpu

ENT_TILE = 1024                 # octree.hip: splats per workgroup of the fused front end
WORD = 64                       # ... and per word of the matrix
SUB = 3
OFFSET = (40, -13, 7)
ROUTES = [6, 8, 3]              # levels: two digits and one word per entry; 22 key bits; one digit


def both_routes(ctx, monkeypatch, cloud, first, n, size, offset, levels):
    """One word per entry between the passes (where the build takes that route), then two."""
    build_and_compare(ctx, cloud, first, n, size, offset, SUB, levels)
    monkeypatch.setenv("MLSGPU_HIP_OCTREE_PACKED", "0")
    build_and_compare(ctx, cloud, first, n, size, offset, SUB, levels)


def mixed(n, levels, size, offset, seed):
    """Splats of every slot mask: saturated ones and splats of every size on and off the grid, shuffled."""
    rng = np.random.default_rng(seed)
    cloud = np.concatenate([tc.corners(n - n // 2, levels, SUB, size, offset, seed), tc.faces(n // 2, levels, SUB, size, offset, seed)])
    return cloud[rng.permutation(n)]


COUNTS = [1, WORD - 1, WORD, WORD + 1, ENT_TILE // 2 - 1, ENT_TILE // 2, ENT_TILE // 2 + 1, ENT_TILE - 1, ENT_TILE,
          ENT_TILE + 1, 2 * ENT_TILE + 1]


@pytest.mark.parametrize("levels", ROUTES)
def test_counts_at_word_and_tile_edges(ctx, levels, monkeypatch):
    """The last word of the matrix, the first half of a tile and the last tile full, one short and one over; the splats
    begin at a ragged firstSplat."""
    size = tc.ragged_size(levels, SUB, cap=256)
    first = 77
    for n in COUNTS:
        both_routes(ctx, monkeypatch, mixed(n + first, levels, size, OFFSET, seed=n + levels), first, n, size, OFFSET, levels)
        monkeypatch.delenv("MLSGPU_HIP_OCTREE_PACKED")


@pytest.mark.parametrize("levels", ROUTES)
def test_tiles_of_one_splat(ctx, levels, monkeypatch):
    """Two tiles and one splat, all the same splat with eight entries: every word of eight digits is full (64 lanes on one
    LDS word), the ranks run to the tile size across every group, and a tile holds as many entries as its array has words."""
    size = tc.ragged_size(levels, SUB, cap=256)
    n = 2 * ENT_TILE + 1
    cloud = np.repeat(tc.corners(1, levels, SUB, size, OFFSET, seed=levels), n)
    assert len(tc.entries(cloud, 0, OFFSET, SUB, levels)) == 8 * n
    both_routes(ctx, monkeypatch, cloud, 0, n, size, OFFSET, levels)


@pytest.mark.parametrize("levels", [6, 3])
def test_runs_without_entries(ctx, levels, monkeypatch):
    """Splats outside the bounds between splats with entries: runs of 1, 63, 64 and 65 inside a tile, from its first splat
    and up to its last, and a whole tile without an entry between two saturated ones."""
    size = tc.ragged_size(levels, SUB, cap=256)
    rng = np.random.default_rng(levels)
    n = 5 * ENT_TILE + 3
    cloud = tc.corners(n, levels, SUB, size, OFFSET, seed=10 + levels)
    far = tc.far_away(n, levels, SUB, size, OFFSET, seed=20 + levels)
    empty = np.zeros(n, bool)
    at = 0
    for run in (1, WORD - 1, WORD, WORD + 1, 1, 2 * WORD):          # tile 0: from its first splat
        empty[at:at + run] = True
        at += run + int(rng.integers(1, 40))
    assert at < ENT_TILE
    empty[ENT_TILE - WORD - 1:ENT_TILE] = True                       # ... and up to its last
    empty[2 * ENT_TILE:3 * ENT_TILE] = True                          # tile 1 full, tile 2 empty, tile 3 full
    empty[4 * ENT_TILE:] = rng.random(n - 4 * ENT_TILE) < 0.5        # tile 4: every other splat or so
    cloud[empty] = far[empty]
    counts = tc.tile_counts(tc.entries(cloud, 0, OFFSET, SUB, levels), 0, n, ENT_TILE)
    assert counts[1] == 8 * ENT_TILE and counts[2] == 0 and counts[3] == 8 * ENT_TILE
    both_routes(ctx, monkeypatch, cloud, 0, n, size, OFFSET, levels)


@pytest.mark.parametrize("levels", [6, 8])
def test_neighbours_across_powers_of_two(ctx, levels, monkeypatch):
    """Eight entries around node corners whose coordinates are powers of two, at every level of the tree that has one (four
    nodes or more to an axis): the lowest node has coordinates 2^j - 1 (odd, all ones) and its neighbours 2^j, so + 1
    carries through every bit the level has.  The keys of a splat still differ in their low three bits."""
    lo, hi = tc.shifts(levels, SUB)
    size = tc.ragged_size(levels, SUB)
    centres, radii, places = [], [], []
    for s in range(lo, hi - 1):
        nodes = 1 << (hi - s)                       # the bounds of a level are the tree's, not the grid's
        powers = [1 << j for j in range(1, 11) if (1 << j) < nodes]
        for kx in powers:
            for ky in powers:
                for kz in powers:
                    centres.append((kx << s, ky << s, kz << s))
                    radii.append((1 << s) / 2.0 - 0.1)
                    places.append((s, kx - 1, ky - 1, kz - 1))
    rng = np.random.default_rng(levels)
    pick = rng.integers(0, len(centres), 2 * ENT_TILE + 77)
    cloud = tc._finish(np.asarray(centres, np.float64)[pick] + np.asarray(OFFSET, np.float64), np.asarray(radii)[pick], rng)
    ent = tc.entries(cloud, 0, OFFSET, SUB, levels)
    assert len(ent) == 8 * len(cloud)
    lowest = ent.rows[0::8, 1:5]
    assert np.array_equal(lowest, np.asarray(places)[pick]) and np.all(lowest[:, 1:] & 1)
    assert len(set(places)) >= 100 and len(set(p[0] for p in places)) == hi - lo - 1
    _, per_pass = tc.digit_bits(levels, SUB)
    digits = (ent.keys() & ((1 << per_pass) - 1)).reshape(-1, 8)
    assert all(len(set(row)) == 8 for row in digits.tolist())
    both_routes(ctx, monkeypatch, cloud, 0, len(cloud), size, OFFSET, levels)


@pytest.mark.parametrize("levels,sub", [(1, 3), (1, 0), (2, 3), (2, 1), (9, 3)])
def test_shallow_and_deep_trees(ctx, levels, sub, monkeypatch):
    """One level: a one-bit digit, where a splat has its slot 0 or nothing.  Two levels: a four-bit digit.  Nine levels:
    25 key bits, more than an LDS word holds beside the splat's place -- the separate passes, as before."""
    from mlsgpu_amd import synth
    key_bits, per_pass = tc.digit_bits(levels, sub)
    assert (key_bits, per_pass) == {1: (1, 1), 2: (4, 4), 9: (25, 9)}[levels]
    size = tc.ragged_size(levels, sub, cap=256)
    n, first = 2 * ENT_TILE + 1, 5
    cloud = synth.uniform_cloud(n + first, float(size[0] + 3), 0.3 * (1 << sub) / 8.0, 9.0 * (1 << sub) / 8.0, seed=levels * 10 + sub)
    cloud["position"] += np.asarray(OFFSET, np.float32) - np.float32(2.0)
    ent = tc.entries(cloud, first, OFFSET, sub, levels)
    per_splat = np.bincount(ent.rows[:, 0] - first, minlength=n)
    assert (per_splat.max() == 1 if levels == 1 else per_splat.max() >= 4) and per_splat.min() == 0
    build_and_compare(ctx, cloud, first, n, size, OFFSET, sub, levels)
    monkeypatch.setenv("MLSGPU_HIP_OCTREE_PACKED", "0")
    build_and_compare(ctx, cloud, first, n, size, OFFSET, sub, levels)


@pytest.mark.parametrize("packed", ["1", "0"])
def test_batch_of_unequal_lanes(ctx, packed, monkeypatch):
    """Lanes of a word, of no splat, of half a tile and one, of a tile and one, of three tiles with an empty one: every lane's
    workgroups rank their own tile and leave where the lane has none."""
    import mlsgpu_amd as m
    monkeypatch.setenv("MLSGPU_HIP_OCTREE_PACKED", packed)
    levels = 6
    size = tc.ragged_size(levels, SUB, cap=256)
    holes = mixed(3 * ENT_TILE, levels, size, OFFSET, seed=5)
    holes[ENT_TILE:2 * ENT_TILE] = tc.far_away(ENT_TILE, levels, SUB, size, OFFSET, seed=6)
    lanes = [(mixed(WORD + 3, levels, size, OFFSET, seed=1), 3, WORD),
             (mixed(4, levels, size, OFFSET, seed=2), 2, 0),
             (tc.corners(ENT_TILE // 2 + 1, levels, SUB, size, OFFSET, seed=3), 0, ENT_TILE // 2 + 1),
             (mixed(ENT_TILE + 1 + 77, levels, size, OFFSET, seed=4), 77, ENT_TILE + 1),
             (holes, 0, len(holes))]
    trees, bufs = [], []
    for cloud, first, n in lanes:
        trees.append(m.SplatTree(ctx, levels, max(n, 1)))
        bufs.append(m.DeviceBuffer(ctx, array=cloud))
    m.SplatTree.build_batch(trees, [(buf, first, n, size, OFFSET) for buf, (_, first, n) in zip(bufs, lanes)], SUB)
    ctx.synchronize()
    for k, (tree, (cloud, first, n)) in enumerate(zip(trees, lanes)):
        t = ob.Tree(cloud.copy(), first, n, size, OFFSET, SUB, levels)
        np.testing.assert_array_equal(tree.start()[:t.num_start], t.start[:t.num_start], err_msg="lane %d start" % k)
        np.testing.assert_array_equal(tree.commands()[:t.num_commands], t.commands[:t.num_commands],
                                      err_msg="lane %d commands" % k)
