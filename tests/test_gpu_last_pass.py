"""The last pass of the octree's entry sort on packed words (commandHistKernel / commandScatterKernel, octree.hip): clouds
chosen by ENTRY count and by where the groups of the first pass (the keys' low parts) fall against the last pass's tiles of
4096 entries.  Every case compares `start` and `commands` word for word with the oracle's tree, on three routes: the last
pass's own kernels, the sort's templates on the same packed words (MLSGPU_HIP_OCTREE_LAST_PASS=0) and two words per entry
(MLSGPU_HIP_OCTREE_PACKED=0).  The builders assert on the host that a cloud has the shape its name says (tc.entries);
test_shapes runs them without a GPU.

Two things the build cannot be made to do from outside, so no case has them:
 - a top digit of 2^bits - 1: the keys of a tree end at numStart - 1 (the root), about 0.57 * 2^keyBits, so the largest top
   digit is (numStart - 1) >> perPass (146 of 255 at six levels, 36 of 63 at five); `extremes` has that one beside digit 0;
 - a device count below the launch's n: on this route the launch is sized by that very count.  `test_one_tree_many_builds`
   leaves the previous build's words behind the end instead.
"""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import tree_cases as tc
from gpu_common import ctx  # noqa: F401
from test_gpu_tree import build_and_compare

TILE = 4096                     # primitives.hpp: SORT_TILE
SLOTS = 4                       # ... KEY_COUNT_SLOTS: low parts a tile counts in LDS
SUB = 3
OFFSET = (40, -13, 7)
FIRST = 77
ROUTES = [{}, {"MLSGPU_HIP_OCTREE_LAST_PASS": "0"}, {"MLSGPU_HIP_OCTREE_PACKED": "0"}]


def all_routes(ctx, monkeypatch, cloud, first, n, levels):
    size = tc.ragged_size(levels, SUB)
    for env in ROUTES:
        with monkeypatch.context() as mp:
            for name in ("MLSGPU_HIP_OCTREE_LAST_PASS", "MLSGPU_HIP_OCTREE_PACKED"):
                mp.delenv(name, raising=False)
            for name, value in env.items():
                mp.setenv(name, value)
            build_and_compare(ctx, cloud, first, n, size, OFFSET, SUB, levels)


def layout(cloud, first, levels):
    """What the last pass reads: (low part, top digit) of every entry in the order the first pass leaves them -- grouped by
    low part, (splat, slot) order inside a group."""
    ent = tc.entries(cloud, first, OFFSET, SUB, levels)
    _, per_pass = tc.digit_bits(levels, SUB)
    keys = ent.keys()
    low = keys & ((1 << per_pass) - 1)
    order = np.argsort(low, kind="stable")
    return low[order], (keys >> per_pass)[order]


def finest_keys(levels):
    """Number of keys of the finest level: Morton codes, no level offset."""
    return 8 ** (levels - 1)


def keyed(keys, levels, seed):
    """One splat with one entry per key of the finest level, in the order given, behind FIRST splats that are skipped."""
    rng = np.random.default_rng(seed)
    keys = np.asarray(keys, np.int64)
    assert keys.min() >= 0 and keys.max() < finest_keys(levels)
    nodes = np.zeros((len(keys), 3), np.int64)
    for b in range(10):
        for axis in range(3):
            nodes[:, axis] |= ((keys >> (3 * b + axis)) & 1) << b
    lo, _ = tc.shifts(levels, SUB)
    size = tc.ragged_size(levels, SUB)
    cloud = np.concatenate([tc.far_away(FIRST, levels, SUB, size, OFFSET, seed + 1), tc._inside_nodes(nodes, lo, OFFSET, rng)])
    ent = tc.entries(cloud, FIRST, OFFSET, SUB, levels)
    assert np.array_equal(ent.keys(), keys) and np.array_equal(ent.rows[:, 0], FIRST + np.arange(len(keys)))
    return cloud


def with_count(levels, count):
    """`count` entries: a saturated cloud of eight entries per splat, topped up with splats of one entry, shuffled."""
    rng = np.random.default_rng(count + levels)
    size = tc.ragged_size(levels, SUB)
    cloud = tc.corners(FIRST + count // 8, levels, SUB, size, OFFSET, seed=count + levels)
    if count % 8:
        cloud = np.concatenate([cloud, tc.one_node(count % 8, levels, SUB, size, OFFSET, seed=count)])
    cloud[FIRST:] = cloud[FIRST:][rng.permutation(len(cloud) - FIRST)]
    assert len(tc.entries(cloud, FIRST, OFFSET, SUB, levels)) == count
    return cloud


def groups(levels, runs, seed):
    """Low part `low` holds `count` entries, for every (low, count) of runs; top digits at random, splats shuffled."""
    rng = np.random.default_rng(seed)
    _, per_pass = tc.digit_bits(levels, SUB)
    tops = finest_keys(levels) >> per_pass
    keys = np.concatenate([rng.integers(0, tops, count) << per_pass | low for low, count in runs])
    cloud = keyed(keys[rng.permutation(len(keys))], levels, seed)
    low, _ = layout(cloud, FIRST, levels)
    assert np.array_equal(low, np.repeat([r[0] for r in runs], [r[1] for r in runs]))
    return cloud


def parts_of_tile(low, tile):
    return len(np.unique(low[tile * TILE:(tile + 1) * TILE]))


# ---------------------------------------------------------------------------------------------------------------------
# the clouds: name -> (cloud, first, levels); every builder asserts the shape it is named for


@functools.lru_cache(maxsize=None)
def shape(name, levels):
    _, per_pass = tc.digit_bits(levels, SUB)
    num_low = 1 << per_pass
    if name == "boundary":
        # group 0 ends exactly on the tile boundary; group 1 is empty and BEGINS on it, group 2 holds all of tile 1; tile 2 is
        # a lane's last and lies across two groups with three empty ones between them
        cloud = groups(levels, [(0, TILE), (2, TILE + 100), (6, 300)], seed=levels)
        low, _ = layout(cloud, FIRST, levels)
        assert low[TILE - 1] == 0 and low[TILE] == 2 and [parts_of_tile(low, t) for t in range(3)] == [1, 1, 2]
        return cloud, FIRST, levels
    if name.startswith("parts"):
        # tile 0 holds k low parts (2, 4 = the slot limit, 5 and more than 8), with empty low parts before, between and after
        k = int(name[5:])
        lows = [3 + 7 * i for i in range(k)]
        total = TILE + 500
        runs = [(low, total // k + (total % k if low == lows[-1] else 0)) for low in lows]
        cloud = groups(levels, runs, seed=10 * levels + k)
        low, _ = layout(cloud, FIRST, levels)
        assert len(low) == total and lows[0] > 0 and lows[-1] < num_low - 1
        assert parts_of_tile(low, 0) == {2: 2, 4: SLOTS, 5: SLOTS + 1, 12: 11}[k] and parts_of_tile(low, 1) <= 2
        return cloud, FIRST, levels
    if name == "one_key":
        # one node: every word of two tiles and one entry has ONE top digit and ONE low part -- a run of 4096, and 64 lanes on
        # one match word in every round
        size = tc.ragged_size(levels, SUB)
        cloud = tc.one_node(FIRST + 2 * TILE + 1, levels, SUB, size, OFFSET, seed=levels)
        low, top = layout(cloud, FIRST, levels)
        assert len(low) == 2 * TILE + 1 and len(np.unique(low)) == 1 and len(np.unique(top)) == 1
        return cloud, FIRST, levels
    if name == "one_top":
        # one top digit under every low part: tiles across many low parts whose words agree in their digit
        size = tc.ragged_size(levels, SUB)
        cloud = tc.one_high_digit(FIRST + 2 * TILE + 1, levels, SUB, size, OFFSET, seed=levels)
        low, top = layout(cloud, FIRST, levels)
        assert len(low) == 2 * TILE + 1 and len(np.unique(top)) == 1 and parts_of_tile(low, 0) > 2 * SLOTS
        return cloud, FIRST, levels
    if name == "once_per_round":
        # one low part, top digits in rotation: the 64 words a wave takes in a round have 64 different digits, in every round
        # of both tiles
        tops = finest_keys(levels) >> per_pass
        assert tops >= 64
        keys = (np.arange(2 * TILE) % tops) << per_pass | 9
        cloud = keyed(keys, levels, seed=levels)
        low, top = layout(cloud, FIRST, levels)
        assert np.all(low == 9) and all(len(set(run)) == 64 for run in top.reshape(-1, 64).tolist())
        return cloud, FIRST, levels
    if name == "extremes":
        # top digit 0 and the largest a tree of these levels has (its root's), around a tile and a half of mixed entries
        size = tc.ragged_size(levels, SUB)
        cloud = with_count(levels, TILE + TILE // 2)
        giant = tc._finish(np.asarray(OFFSET, np.float64) + np.asarray(size) / 2.0, [size[0] * 0.4], np.random.default_rng(1))
        cloud = np.concatenate([cloud, keyed([0, 1], levels, seed=3)[FIRST:], giant])
        _, top = layout(cloud, FIRST, levels)
        num_start = (8 ** levels - 1) // 7
        assert top.min() == 0 and top.max() == (num_start - 1) >> per_pass
        return cloud, FIRST, levels
    raise KeyError(name)


SHAPES = [(name, levels) for levels in (6, 5)
          for name in ("boundary", "parts2", "parts4", "parts5", "parts12", "one_key", "one_top", "extremes")]
SHAPES.append(("once_per_round", 6))       # (five levels have 32 top digits on the finest level: no 64 different ones)
COUNTS = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


def shallow(levels):
    """Trees of one to three levels: the key has ONE digit, the last pass's top digit has zero bits (one bin)."""
    from mlsgpu_amd import synth
    key_bits, per_pass = tc.digit_bits(levels, SUB)
    assert key_bits == per_pass == {1: 1, 2: 4, 3: 7}[levels]
    size = tc.ragged_size(levels, SUB)
    n, first = (3 * TILE if levels == 1 else TILE), 5
    cloud = synth.uniform_cloud(n + first, float(size[0] + 3), 0.3, 9.0, seed=levels)
    cloud["position"] += np.asarray(OFFSET, np.float32) - np.float32(2.0)
    low, top = layout(cloud, first, levels)
    assert len(low) > TILE + 64 and np.all(top == 0) and (levels == 1 or parts_of_tile(low, 0) >= 2)
    return cloud, first


def unequal_lanes(levels):
    """(cloud, first, n) per lane: no splat, fewer entries than a wave, one tile and one entry, three tiles (the last short)."""
    lanes = [(with_count(levels, 8), 2, 0),
             (with_count(levels, 37), FIRST, None),
             (with_count(levels, TILE + 1), FIRST, None),
             (groups(levels, [(1, TILE + 9), (2, 70), (100, TILE + 800)], seed=40 + levels), FIRST, None)]
    lanes = [(cloud, first, len(cloud) - first if n is None else n) for cloud, first, n in lanes]
    counts = [len(tc.entries(cloud, first, OFFSET, SUB, levels, n)) for cloud, first, n in lanes]
    assert counts == [0, 37, TILE + 1, 2 * TILE + 879]
    return lanes


def test_shapes():
    """Every cloud has the shape it is named for (the builders' own assertions): no GPU."""
    for name, levels in SHAPES:
        shape(name, levels)
    for levels in (6, 5):
        for count in COUNTS:
            with_count(levels, count)
        unequal_lanes(levels)
    for levels in (1, 2, 3):
        shallow(levels)


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [6, 5])
def test_counts_at_tile_edges(ctx, levels, monkeypatch):
    """Six levels (8 + 8 bits, the headline's route) and five (7 + 6): one entry, a wave's round one short, full and one
    over, the tile one short, full and one over, two tiles and one entry; ragged firstSplat."""
    for count in COUNTS:
        cloud = with_count(levels, count)
        all_routes(ctx, monkeypatch, cloud, FIRST, len(cloud) - FIRST, levels)


@pytest.mark.gpu
@pytest.mark.parametrize("name,levels", SHAPES)
def test_low_parts_and_digits(ctx, name, levels, monkeypatch):
    """Low parts against tiles, and the digits of a tile: see `shape`."""
    cloud, first, levels = shape(name, levels)
    all_routes(ctx, monkeypatch, cloud, first, len(cloud) - first, levels)


@pytest.mark.gpu
@pytest.mark.parametrize("levels", [1, 2, 3])
def test_shallow_trees(ctx, levels, monkeypatch):
    """A top digit of zero bits: the last pass's own kernels serve it, with one bin."""
    cloud, first = shallow(levels)
    all_routes(ctx, monkeypatch, cloud, first, len(cloud) - first, levels)


@pytest.mark.gpu
@pytest.mark.parametrize("route", range(len(ROUTES)))
def test_batch_of_unequal_lanes(ctx, route, monkeypatch):
    """Workgroups beyond a lane's tiles leave at once, and every lane ranks only its own tiles."""
    import mlsgpu_amd as m
    for name, value in ROUTES[route].items():
        monkeypatch.setenv(name, value)
    levels = 6
    size = tc.ragged_size(levels, SUB)
    lanes = unequal_lanes(levels)
    trees = [m.SplatTree(ctx, levels, max(n, 1)) for _, _, n in lanes]
    bufs = [m.DeviceBuffer(ctx, array=cloud) for cloud, _, _ in lanes]
    m.SplatTree.build_batch(trees, [(buf, first, n, size, OFFSET) for buf, (_, first, n) in zip(bufs, lanes)], SUB)
    ctx.synchronize()
    for k, (tree, (cloud, first, n)) in enumerate(zip(trees, lanes)):
        t = ob.Tree(cloud.copy(), first, n, size, OFFSET, SUB, levels)
        np.testing.assert_array_equal(tree.start()[:t.num_start], t.start[:t.num_start], err_msg="lane %d start" % k)
        np.testing.assert_array_equal(tree.commands()[:t.num_commands], t.commands[:t.num_commands], err_msg="lane %d commands" % k)


@pytest.mark.gpu
@pytest.mark.parametrize("route", range(len(ROUTES)))
def test_one_tree_many_builds(ctx, route, monkeypatch):
    """A large cloud, then small ones in the same tree: the words of the large build stay behind the small builds' end and
    are not counted."""
    import mlsgpu_amd as m
    from test_gpu_tree import build_on, compare_with_oracle
    for name, value in ROUTES[route].items():
        monkeypatch.setenv(name, value)
    levels = 6
    size = tc.ragged_size(levels, SUB)
    clouds = [with_count(levels, 4 * TILE + 8), with_count(levels, TILE + 1), with_count(levels, 65), shape("parts5", levels)[0],
              with_count(levels, 1)]
    tree = m.SplatTree(ctx, levels, max(len(c) for c in clouds))
    for cloud in clouds:
        n = len(cloud) - FIRST
        commands, start, num_levels, after = build_on(tree, ctx, cloud, FIRST, n, size, OFFSET, SUB)
        assert num_levels == levels
        compare_with_oracle(commands, start, after, cloud, FIRST, n, size, OFFSET, SUB, levels)
