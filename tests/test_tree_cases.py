"""The octree's numpy anchor (tree_cases.py): its clouds do what they are for, and the oracle's tree holds, leaf by leaf,
exactly what the brute force says -- on saturated, skewed, face-straddling and far-corner clouds, up to levels 10."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import tree_cases as tc
from refdata import walk

DEFAULT = (6, 3, (256, 251, 248), (40, -13, 7))
FIRST = 77
N = 5077                        # four whole tiles of 1024 splats and a ragged one
N_FACES = 20_000                # room for two far runs

ORACLE_CASES = [(name,) + DEFAULT for name in ("corners", "one_node", "one_low_digit", "one_high_digit", "faces", "far_corner")]
ORACLE_CASES.append(("faces", 6, 2, (128, 120, 99), (-5, 9, 100)))
ORACLE_CASES += [("far_corner", levels, sub, tc.ragged_size(levels, sub), (2, -7, 1))
                 for levels, sub in ((7, 3), (8, 3), (9, 3), (10, 3), (10, 0), (6, 5))]


@functools.lru_cache(maxsize=None)
def case(name, levels, sub, size, offset):
    """(cloud, n, entries) of a case; the cloud's first FIRST splats are not part of the build."""
    n = N_FACES if name == "faces" else N
    cloud = tc.BUILDERS[name](n + FIRST, levels, sub, size, offset, seed=len(name) + 10 * levels + sub)
    cloud.setflags(write=False)
    return cloud, n, tc.entries(cloud, FIRST, offset, sub, levels)


def digits(ent, levels, sub):
    """(first-pass digit, what lies above it) of every entry's key."""
    _, per_pass = tc.digit_bits(levels, sub)
    keys = ent.keys()
    return keys & ((1 << per_pass) - 1), keys >> per_pass


def test_builders_do_what_they_are_for():
    levels, sub = DEFAULT[:2]
    cloud, n, ent = case("corners", *DEFAULT)
    assert np.array_equal(np.bincount(ent.rows[:, 0] - FIRST, minlength=n), np.full(n, 8))
    tiles = tc.tile_counts(ent, FIRST, n)
    assert len(ent) / n == 8.0 and (tiles == 8192).sum() >= 1
    assert (tiles[:-1] == 8192).all()                   # no slack: every whole tile fills the scatter kernel's LDS array
    for name, low, high in (("one_node", (1, 1), (1, 1)), ("one_low_digit", (1, 1), (50, None)),
                            ("one_high_digit", (200, None), (1, 1))):
        cloud, n, ent = case(name, *DEFAULT)
        assert np.array_equal(ent.rows[:, 0], np.arange(FIRST, FIRST + n)), name       # one entry per splat
        assert (ent.rows[:, 1] == sub).all()
        lo, hi = (len(np.unique(d)) for d in digits(ent, levels, sub))
        assert low[0] <= lo and (low[1] is None or lo <= low[1]), (name, lo)
        assert high[0] <= hi and (high[1] is None or hi <= high[1]), (name, hi)
    cloud, n, ent = case("faces", *DEFAULT)
    runs = tc.far_runs(n + FIRST)
    assert len(runs) == 2
    made = np.bincount(ent.rows[:, 0], minlength=n + FIRST)
    for b, e in runs:
        assert e - b >= 2048 and b >= FIRST and not made[b:e].any()
        assert made[b - 1024:b].any() and made[e:e + 1024].any()        # ... between populated tiles
    assert np.abs(cloud["position"]).max() < 2 ** 24 and np.isfinite(cloud["position"]).all()
    # both clamps of the level: the finest (far smaller than a cell) and the coarsest (larger than the grid, one node)
    assert {sub, sub + levels - 1} <= set(np.unique(ent.rows[:, 1]).tolist())
    per_splat = np.bincount(ent.rows[:, 0], minlength=n + FIRST)[FIRST:]
    assert 0 < per_splat[per_splat > 0].min() and per_splat.max() == 8 and (per_splat == 0).sum() > 4096
    for name in tc.BUILDERS:
        cloud = case(name, *DEFAULT)[0] if name != "far_away" else tc.far_away(3000, *DEFAULT, seed=5)
        nrm = cloud["normal"].astype(np.float64)
        np.testing.assert_allclose((nrm * nrm).sum(axis=1), 1.0, atol=1e-6)
        assert (cloud["quality"] >= 0.5).all() and (cloud["quality"] <= 2.0).all() and (cloud["radius"] > 0).all()
    assert len(tc.entries(tc.far_away(3000, *DEFAULT, seed=5), 0, DEFAULT[3], sub, levels)) == 0


def test_uniform_cloud_leaves_tiles_half_empty():
    """For contrast: the cloud of test_gpu_tree.test_parity_default_geometry fills no tile."""
    from mlsgpu_amd import synth
    n, first = 200_000, 1234
    cloud = synth.uniform_cloud(n + first, 255.0, 0.5, 9.0, seed=77)
    cloud["position"] += np.float32(40.0)
    ent = tc.entries(cloud, first, (40, 40, 40), 3, 6)
    tiles = tc.tile_counts(ent, first, n)
    print("uniform cloud: %.3f entries per splat, fullest tile %d of 8192" % (len(ent) / n, tiles.max()))
    assert 3.5 < len(ent) / n < 4.5 and tiles.max() < 8192 * 10 // 16          # never past round 10 of 16


def walk_ids(commands, pos):
    """refdata.walk with its checks, a node's ids taken as one slice (a coarse node of `faces` lists thousands)."""
    parts, steps = [np.zeros(0, np.int64)], 0
    while pos >= 0:
        end = int(commands[pos])
        assert pos + 1 < end < len(commands), "bad end pointer"
        parts.append(commands[pos + 1:end])
        pos = int(commands[end])
        assert pos >= -1
        steps += 1
        assert steps <= 32, "more nodes on a walk than the tree has levels"
    return np.concatenate(parts)


def test_walk_ids_is_refdata_walk():
    name, levels, sub, size, offset = ORACLE_CASES[4]
    cloud, n, ent = case(name, levels, sub, size, offset)
    t = ob.Tree(cloud.copy(), FIRST, n, size, offset, sub, levels)
    seen = 0
    for key in range(0, 32 ** 3, 97):
        if t.start[key] != -1:
            assert walk_ids(t.commands, int(t.start[key])).tolist() == walk(t.commands, t.start[key])
            seen += 1
    assert seen > 100


def leaves_to_check(ent, levels, sub, size, seed):
    min_shift, max_shift = ent.min_shift, ent.max_shift
    side = 1 << (max_shift - min_shift)
    if side ** 3 <= 40_000:                                     # the whole cube of leaves, the grid's among them
        g = np.arange(side)
        return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    per_axis = (np.asarray(size, np.int64) + (1 << min_shift) - 1) >> min_shift
    if per_axis.prod() <= 40_000:
        return np.stack(np.meshgrid(*[np.arange(k) for k in per_axis], indexing="ij"), -1).reshape(-1, 3)
    up = (ent.rows[:, 1] - min_shift)[:, None]
    node = ent.rows[:, 2:5]
    cornered = np.unique(np.concatenate([node << up, ((node + 1) << up) - 1]), axis=0)
    rng = np.random.default_rng(seed)
    if len(cornered) <= 4000:
        return cornered
    picked = cornered[rng.choice(len(cornered), 3500, replace=False)]
    return np.concatenate([picked, rng.integers(0, per_axis, (500, 3))])


@pytest.mark.parametrize("name,levels,sub,size,offset", ORACLE_CASES,
                         ids=["%s-%d-%d" % c[:3] + ("-small" if c[3][0] == 128 else "") for c in ORACLE_CASES])
def test_oracle_tree_equals_brute_force(name, levels, sub, size, offset):
    cloud, n, ent = case(name, levels, sub, size, offset)
    mutated = cloud.copy()
    t = ob.Tree(mutated, FIRST, n, size, offset, sub, levels)
    assert t.num_levels == levels
    leaves = leaves_to_check(ent, levels, sub, size, seed=levels + sub)
    keys = tc.morton(*leaves.T)
    starts = t.start[keys]
    wrong = 0
    for leaf, pos in zip(leaves.tolist(), starts.tolist()):
        wrong += not np.array_equal(walk_ids(t.commands, pos), tc.expected_walk(ent, leaf))
    assert wrong == 0, "%d of %d leaves" % (wrong, len(leaves))
    # radius -> 1 / r^2 inside the range, nothing outside it
    r = cloud["radius"][FIRST:]
    np.testing.assert_array_equal(mutated["radius"][FIRST:], np.float32(1.0) / (r * r))
    np.testing.assert_array_equal(mutated[:FIRST].view(np.uint32), cloud[:FIRST].view(np.uint32))
