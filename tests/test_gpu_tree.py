"""SplatTreeCL on the GPU: the reference's own assertions (test/test_splat_tree*.cpp) and bit parity with the oracle."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import tree_cases as tc
from gpu_common import ctx  # noqa: F401
from refdata import make_splats
from test_oracle_tree import BUILD_SPLATS, check_build, check_random, random_splats

pytestmark = pytest.mark.gpu


def test_make_code(ctx):
    import mlsgpu_amd as m
    out = C.c_uint32()
    for xyz, exp in [((0, 0, 0), 0), ((1, 1, 1), 7), ((2, 5, 3), 174), ((7, 7, 7), 511), ((123, 456, 789), 642569997)]:
        m.binding.check(m.lib().mlsgpu_hip_test_make_code(ctx.h, *xyz, C.byref(out)))
        assert out.value == exp


def test_level_shift(ctx):
    import mlsgpu_amd as m
    cases = [(0, (0, 0, 0), (0, 0, 0)), (0, (1, 1, 1), (0, 0, 0)), (0, (0, 1, 2), (1, 2, 3)),
             (1, (0, 1, 2), (2, 2, 3)), (1, (0, 1, 2), (1, 3, 3)), (1, (0, 1, 2), (1, 2, 4)),
             (2, (31, 0, 0), (35, 0, 0)), (3, (31, 0, 0), (36, 0, 0)), (3, (27, 0, 0), (32, 0, 0)),
             (5, (48, 0, 0), (79, 0, 0))]
    out = C.c_int32()
    for exp, lo, hi in cases:
        m.binding.check(m.lib().mlsgpu_hip_test_level_shift(ctx.h, ob._p(np.array(lo, np.int32)),
                                                             ob._p(np.array(hi, np.int32)), C.byref(out)))
        assert out.value == exp


def test_point_box_dist2(ctx):
    import mlsgpu_amd as m
    cases = [(0.0, (0.5, 0.5, 0.5), (0, 0, 0), (1, 1, 1)),
             (4.0, (0.25, 0.5, 3.0), (-1.5, 0.0, 0.5), (1.5, 0.75, 1.0)),
             (14.0, (9.0, 11.0, -10.0), (-1.0, 0.0, -7.0), (8.0, 9.0, 8.0))]
    out = C.c_float()
    for exp, p, lo, hi in cases:
        arrs = [np.array(v, np.float32) for v in (p, lo, hi)]
        m.binding.check(m.lib().mlsgpu_hip_test_point_box_dist2(ctx.h, *[ob._p(a) for a in arrs], C.byref(out)))
        assert abs(out.value - exp) < 1e-4


def build_on(tree, ctx, splats, first, num, size, offset, subsampling):
    """One build of an existing tree on a fresh copy of `splats`: (commands, start, numLevels, the splats afterwards)."""
    import mlsgpu_amd as m
    buf = m.DeviceBuffer(ctx, array=splats)
    tree.enqueue_build(buf, first, num, size, offset, subsampling)
    ctx.synchronize()
    return tree.commands(), tree.start(), tree.num_levels, buf.download(m.SPLAT_DTYPE, len(splats))


def gpu_build(ctx, splats, first, num, size, offset, subsampling, levels, max_splats=None, mutate=True):
    import mlsgpu_amd as m
    tree = m.SplatTree(ctx, levels, max_splats or max(len(splats), 1))
    if not mutate:
        tree.set_mutate(False)
    return build_on(tree, ctx, splats, first, num, size, offset, subsampling)


def compare_with_oracle(commands, start, mutated, splats, first, num, size, offset, subsampling, levels, mutate=True):
    """Every word of start and commands, and of the splats: mutated as the oracle mutates them, or (mutate=False) untouched."""
    s2 = splats.copy()
    t = ob.Tree(s2, first, num, size, offset, subsampling, levels)
    np.testing.assert_array_equal(start[:t.num_start], t.start[:t.num_start])
    np.testing.assert_array_equal(commands[:t.num_commands], t.commands[:t.num_commands])
    np.testing.assert_array_equal(mutated.view(np.uint32), (s2 if mutate else splats).view(np.uint32))


def test_build_without_mutation(ctx):
    """mlsgpu_hip_tree_set_mutate(0): the same commands / start, and the splats are left as they came."""
    import mlsgpu_amd as m
    from mlsgpu_amd import synth
    cloud, g = synth.make_cloud("cfg1", scale=0.5)
    tree = m.SplatTree(ctx, 6, len(cloud))
    tree.set_mutate(False)
    buf = m.DeviceBuffer(ctx, array=cloud)
    tree.enqueue_build(buf, 0, len(cloud), (64, 64, 64), (0, 0, 0), 3)
    ctx.synchronize()
    t = ob.Tree(cloud.copy(), 0, len(cloud), (64, 64, 64), (0, 0, 0), 3, 6)
    np.testing.assert_array_equal(tree.start()[:t.num_start], t.start[:t.num_start])
    np.testing.assert_array_equal(tree.commands()[:t.num_commands], t.commands[:t.num_commands])
    np.testing.assert_array_equal(buf.download(m.SPLAT_DTYPE, len(cloud)).view(np.uint32), cloud.view(np.uint32))


def test_build(ctx):
    """TestSplatTree::testBuild on the device result."""
    splats = make_splats(BUILD_SPLATS)
    commands, start, num_levels, mutated = gpu_build(ctx, splats, 0, len(splats), (16, 16, 12), (3, 0, 1), 0, 9,
                                                     max_splats=1001)
    check_build(splats, commands, start, num_levels)
    compare_with_oracle(commands, start, mutated, splats, 0, len(splats), (16, 16, 12), (3, 0, 1), 0, 9)


def test_random(ctx):
    """TestSplatTree::testRandom on the device result."""
    splats, cells = random_splats()
    commands, start, _, mutated = gpu_build(ctx, splats, 0, len(splats), cells, (1, 2, -1), 2, 8, max_splats=1000)
    check_random(commands, start, len(splats), cells, 2)
    compare_with_oracle(commands, start, mutated, splats, 0, len(splats), cells, (1, 2, -1), 2, 8)


@pytest.mark.parametrize("n,first", [(0, 0), (1, 0), (5000, 0), (200_000, 1234)])
def test_parity_default_geometry(ctx, n, first):
    """levels 6 / subsampling 3 (the reference defaults) on a 256-corner bucket, ragged sizes, firstSplat > 0."""
    from mlsgpu_amd import synth
    cloud = synth.uniform_cloud(n + first, 255.0, 0.5, 9.0, seed=77)   # radii span several octree levels
    cloud["position"] += np.float32(40.0)                              # bucket offset below
    commands, start, _, mutated = gpu_build(ctx, cloud, first, n, (256, 256, 256), (40, 40, 40), 3, 6)
    compare_with_oracle(commands, start, mutated, cloud, first, n, (256, 256, 256), (40, 40, 40), 3, 6)


def test_argument_checks(ctx):
    import mlsgpu_amd as m
    with pytest.raises(m.LengthError):
        m.SplatTree(ctx, 11, 100)                   # MAX_LEVELS
    with pytest.raises(m.LengthError):
        m.SplatTree(ctx, 6, 0)
    tree = m.SplatTree(ctx, 6, 100)
    buf = m.DeviceBuffer(ctx, array=make_splats(BUILD_SPLATS))
    with pytest.raises(m.LengthError):
        tree.enqueue_build(buf, 0, 101, (8, 8, 8), (0, 0, 0), 3)        # numSplats > maxSplats
    with pytest.raises(m.LengthError):
        tree.enqueue_build(buf, 0, 8, (257, 8, 8), (0, 0, 0), 3)        # size > 2^(levels+sub-1)


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_tree_depth(ctx, levels):
    """Every route of the build: one-digit keys whose only pass is the fused one (levels <= 3: the last pass has nothing left
    to sort, only the command positions to hand out), two digits (the default: whole-key counts in the last pass's histogram
    kernel, a scan over the nodes, ids scattered to their command positions), and deeper trees that keep the scan over the
    entries.  `start` / `commands` equal the oracle's word for word."""
    from mlsgpu_amd import synth
    side = min(1 << (levels + 2), 256)
    cloud = synth.uniform_cloud(30_000, float(side - 1), 0.5, 6.0, seed=1000 + levels)
    size = (side, side - 5, side - 8) if side > 8 else (side, side, side)
    commands, start, num_levels, mutated = gpu_build(ctx, cloud, 0, len(cloud), size, (2, 0, 1), 3, levels)
    compare_with_oracle(commands, start, mutated, cloud, 0, len(cloud), size, (2, 0, 1), 3, levels)


@pytest.mark.parametrize("levels", [2, 6])
def test_two_words_per_entry_route(ctx, levels, monkeypatch):
    """The default route keeps ONE word per entry between the two passes of the entry sort (the low digit is the entry's
    position, the rest of the key sits above the splat's number inside the bucket); MLSGPU_HIP_OCTREE_PACKED=0 is the
    two-word form it replaced -- and what a bucket whose key and splat number do not fit a word together falls back to."""
    from mlsgpu_amd import synth
    monkeypatch.setenv("MLSGPU_HIP_OCTREE_PACKED", "0")
    side = min(1 << (levels + 2), 256)
    cloud = synth.uniform_cloud(40_000 + 77, float(side - 1), 0.5, 6.0, seed=2000 + levels)
    size = (side, side - 5, side - 8) if side > 8 else (side, side, side)
    commands, start, _, mutated = gpu_build(ctx, cloud, 77, 40_000, size, (2, 0, 1), 3, levels)
    compare_with_oracle(commands, start, mutated, cloud, 77, 40_000, size, (2, 0, 1), 3, levels)


# ---------------------------------------------------------------------------------------------------------------------
# Where a uniform cloud never goes (tests/tree_cases.py; tests/test_tree_cases.py pins the oracle on these clouds to a
# brute force): tiles of the fused front end without a free slot, every entry in one node or one digit, splats on and
# beyond every face of the grid, keys with every bit set, trees of 9 and 10 levels, lanes of a batch that differ in kind.

OFFSET = (40, -13, 7)


def build_and_compare(ctx, cloud, first, n, size, offset, sub, levels, mutate=True):
    commands, start, num_levels, after = gpu_build(ctx, cloud, first, n, size, offset, sub, levels, mutate=mutate)
    assert num_levels == levels
    compare_with_oracle(commands, start, after, cloud, first, n, size, offset, sub, levels, mutate=mutate)


@pytest.mark.parametrize("n,first", [(1, 0), (2, 1), (511, 0), (1023, 77), (1024, 0), (1025, 1), (2049, 77), (5077, 77)])
@pytest.mark.parametrize("levels", [3, 5, 6, 8, 4, 7])
def test_saturated_tiles(ctx, levels, n, first, monkeypatch):
    """Eight entries from every splat: a whole tile of the fused front end (levels 3, 5, 6, 8) fills entryScatterKernel's
    LDS array to the last word and runs all 16 of its rounds, and the entry count lies on and either side of the sort's tile
    (1024 splats = 2 x 4096 entries).  Levels 4 and 7 take the unfused route.  At levels 5 and 6 also with two words per
    entry, and without mutation: the splats come back as they went."""
    sub = 3
    size = tc.ragged_size(levels, sub, cap=256)
    cloud = tc.corners(n + first, levels, sub, size, OFFSET, seed=100 * levels + n)
    build_and_compare(ctx, cloud, first, n, size, OFFSET, sub, levels)
    if levels in (5, 6):
        build_and_compare(ctx, cloud, first, n, size, OFFSET, sub, levels, mutate=False)
        monkeypatch.setenv("MLSGPU_HIP_OCTREE_PACKED", "0")
        build_and_compare(ctx, cloud, first, n, size, OFFSET, sub, levels)
        build_and_compare(ctx, cloud, first, n, size, OFFSET, sub, levels, mutate=False)


SKEWED = [(name, levels) for levels in (3, 6, 8) for name in ("one_node", "one_low_digit", "one_high_digit")]
SKEWED += [("one_node", 4), ("one_node", 9)]


@pytest.mark.parametrize("name,levels", SKEWED)
def test_skewed_keys(ctx, name, levels):
    """20 000 entries with one key (one LDS bin, one match word and one node counter take them all), with one first-pass
    digit and many above it, and with every first-pass digit and one above."""
    sub, n, first = 3, 20_000, 77
    size = tc.ragged_size(levels, sub)
    cloud = tc.BUILDERS[name](n + first, levels, sub, size, OFFSET, seed=levels)
    build_and_compare(ctx, cloud, first, n, size, OFFSET, sub, levels)


@pytest.mark.parametrize("levels,sub", [(6, 3), (6, 2), (8, 3), (5, 4)])
def test_grid_faces(ctx, levels, sub):
    """Splats across the low face, on the high face, larger than the grid, far smaller than a cell, and whole tiles without
    an entry between populated ones."""
    n, first, offset = 20_000, 77, (300, -170, 90)
    size = tc.ragged_size(levels, sub)
    cloud = tc.faces(n + first, levels, sub, size, offset, seed=10 * levels + sub)
    build_and_compare(ctx, cloud, first, n, size, offset, sub, levels)


@pytest.mark.parametrize("levels,sub", [(7, 3), (8, 3), (9, 3), (6, 5), (10, 3)])
def test_far_corner_keys(ctx, levels, sub):
    """The largest grid of every pair, the cloud in its far corner: every bit of the key is live (22 at levels 8, where the
    fused route packs the key below the splat's place in the tile), and trees of 9 and 10 levels (25 and 28 key bits; the
    10-level tree and the oracle's hold 600 MB of `start` each -- the one case here that takes more than a moment)."""
    n, first, offset = 20_000, 77, (2, -7, 1)
    size = tc.ragged_size(levels, sub)
    cloud = tc.far_corner(n + first, levels, sub, size, offset, seed=10 * levels + sub)
    build_and_compare(ctx, cloud, first, n, size, offset, sub, levels)


def test_one_tree_many_builds(ctx):
    """One tree, build after build of different kinds: nothing of the previous build shows (node counters, jump slots,
    notes, the entry count)."""
    import mlsgpu_amd as m
    levels, sub, cap = 6, 3, 20_000
    tree = m.SplatTree(ctx, levels, cap)
    size, other = tc.ragged_size(levels, sub), (200, 256, 131)
    builds = [(tc.corners(5077 + 77, levels, sub, size, OFFSET, 1), 77, 5077, size, OFFSET),
              (tc.corners(10, levels, sub, size, OFFSET, 2), 3, 0, size, OFFSET),
              (tc.one_node(cap, levels, sub, size, OFFSET, 3), 0, cap, size, OFFSET),
              (tc.far_away(3000, levels, sub, size, OFFSET, 4), 0, 3000, size, OFFSET),
              (tc.faces(cap, levels, sub, size, OFFSET, 5), 1, cap - 1, size, OFFSET),
              (tc.corners(4096, levels, sub, other, (-3, 500, 0), 6), 0, 4096, other, (-3, 500, 0))]
    for cloud, first, n, sz, off in builds:
        commands, start, num_levels, after = build_on(tree, ctx, cloud, first, n, sz, off, sub)
        assert num_levels == levels
        compare_with_oracle(commands, start, after, cloud, first, n, sz, off, sub, levels)


def mixed_lanes(levels, sub):
    """(cloud, first, n, size, offset, mutate) per lane: saturated, empty, one key, one splat, uniform, no entries, faces,
    saturated with one splat in its second tile."""
    from mlsgpu_amd import synth
    big = tc.ragged_size(levels, sub)
    small = tc.ragged_size(levels, sub, cap=128)
    uniform = synth.uniform_cloud(30_000, float(small[0] - 1), 0.5, 6.0, seed=31)
    uniform["position"] += np.array((7, 7, 7), np.float32)
    return [(tc.corners(5077 + 77, levels, sub, big, OFFSET, 11), 77, 5077, big, OFFSET, True),
            (tc.corners(4, levels, sub, small, (1, 2, 3), 12), 2, 0, small, (1, 2, 3), True),
            (tc.one_node(9000, levels, sub, big, (-40, 0, 9), 13), 0, 9000, big, (-40, 0, 9), False),
            (tc.corners(1, levels, sub, small, (5, 5, -5), 14), 0, 1, small, (5, 5, -5), True),
            (uniform, 0, len(uniform), small, (7, 7, 7), True),
            (tc.far_away(3000, levels, sub, big, (0, 0, 0), 15), 0, 3000, big, (0, 0, 0), True),
            (tc.faces(12_000, levels, sub, (big[2], big[0], big[1]), (300, -170, 90), 16), 5, 11_990, (big[2], big[0], big[1]),
             (300, -170, 90), False),
            (tc.corners(1025, levels, sub, small, (-1, -2, -3), 17), 0, 1025, small, (-1, -2, -3), True)]


@pytest.mark.parametrize("levels", [6, 8])
def test_build_batch_mixed_lanes(ctx, levels):
    """mlsgpu_hip_tree_build_batch itself, on lanes that differ in kind, in size, in offset and in whether they mutate: every
    lane's tree is that lane's alone.  Then a batch whose first lane -- whose mailbox serves the batch -- is the empty one."""
    import mlsgpu_amd as m
    sub = 3
    lanes = mixed_lanes(levels, sub)
    assert len(lanes) == m.binding.MAX_BATCH
    expected = [None] * len(lanes)
    for pick in (list(range(len(lanes))), [1, 2, 7]):
        trees, bufs = [], []
        for k in pick:
            cloud, first, n, size, offset, mutate = lanes[k]
            trees.append(m.SplatTree(ctx, levels, max(n, 1)))
            trees[-1].set_mutate(mutate)
            bufs.append(m.DeviceBuffer(ctx, array=cloud))
        m.SplatTree.build_batch(trees, [(buf,) + lanes[k][1:5] for k, buf in zip(pick, bufs)], sub)
        ctx.synchronize()
        for k, tree, buf in zip(pick, trees, bufs):
            cloud, first, n, size, offset, mutate = lanes[k]
            if expected[k] is None:
                s2 = cloud.copy()
                t = ob.Tree(s2, first, n, size, offset, sub, levels)
                expected[k] = (t.start[:t.num_start], t.commands[:t.num_commands], s2 if mutate else cloud)
            exp_start, exp_commands, exp_splats = expected[k]
            assert tree.num_levels == levels
            np.testing.assert_array_equal(tree.start()[:len(exp_start)], exp_start, err_msg="lane %d start" % k)
            np.testing.assert_array_equal(tree.commands()[:len(exp_commands)], exp_commands, err_msg="lane %d commands" % k)
            np.testing.assert_array_equal(buf.download(m.SPLAT_DTYPE, len(cloud)).view(np.uint32), exp_splats.view(np.uint32),
                                          err_msg="lane %d splats" % k)


def test_saturated_lists_through_process_corners(ctx):
    """The command lists of a saturated tree are walked by processCorners: the GPU tree's own commands / start under the
    two MLS kernels give the oracle's field on the oracle's tree, bit for bit and NaN for NaN."""
    import mlsgpu_amd as m
    levels, sub, n, size, offset = 6, 3, 3000, (64, 64, 64), (40, -13, 7)
    cloud = tc.corners(n, levels, sub, size, offset, seed=64)
    s2 = cloud.copy()
    t = ob.Tree(s2, 0, n, size, offset, sub, levels)
    rows, pitch = 64 * 64, 64
    exp = np.full((rows, pitch), -7.0, np.float32)
    ob.process_corners(exp, s2, t.commands, t.start, sub, offset, 64, 64, 64, 0, 0, 63, ob.lib().orc_boundary_factor(1.0), 0)
    finite = int(np.isfinite(exp).sum())
    print("finite corners: %d of %d" % (finite, exp.size))
    assert exp.size == 262_144 and finite >= 500
    tree = m.SplatTree(ctx, levels, n)
    buf = m.DeviceBuffer(ctx, array=cloud)
    tree.enqueue_build(buf, 0, n, size, offset, sub)
    dfield = m.DeviceBuffer(ctx, array=np.full((rows, pitch), -7.0, np.float32))
    sw = m.Swathe(64, 64, 64, 0, 0, 63)
    for variant in (5, 1):
        gen = m.MlsFunctor(ctx, 0)
        gen.set(offset, tree, sub)
        gen.set_variant(variant)
        dfield.upload(np.full((rows, pitch), -7.0, np.float32))
        gen.enqueue(dfield, pitch, rows, sw)
        ctx.synchronize()
        got = dfield.download(np.float32).reshape(rows, pitch)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg="variant %d" % variant)
        ok = ~np.isnan(exp)
        np.testing.assert_array_equal(got[ok].view(np.uint32), exp[ok].view(np.uint32), err_msg="variant %d" % variant)
