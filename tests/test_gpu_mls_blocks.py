"""processCorners block by block: every octree leaf has a command list of its own, with splats near that leaf only, so a
workgroup that takes another block's place, list or bounds (variant 5 reads all three from its entry of the launch's
descriptor table) computes a visibly different field.  Some leaves have no list (start = -1) and some lists end in a jump to a
run that they share.  Bit-equal, NaN for NaN, to the CPU oracle and to variant 1, which finds a block's place by itself."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_binding as ob
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.0)


def morton(x, y, z):
    """makeCode, kernels/mls.cl:159-174: x in bits 0, 3, .., y in 1, 4, .., z in 2, 5, .."""
    code = 0
    for b in range(10):
        code |= ((x >> b) & 1) << (3 * b) | ((y >> b) & 1) << (3 * b + 1) | ((z >> b) & 1) << (3 * b + 2)
    return code


def blocks_fixture(size, offset, subsampling=3, z_first=0, z_stride=None, z_bias=0, per_leaf=64, seed=1):
    """A grid of size[0] x size[1] corners and slices z_first .. z_first + size[2] - 1.  Leaf (i, j, k) covers the cells
    [i, i + 1) x .. << subsampling; its run lists `per_leaf` splats inside it (support 2 - 3.5 cells: they reach the
    neighbouring blocks' corners too, which those blocks' lists do not know about).  Every fifth leaf has no list, every
    third list jumps to a shared run of splats with a wide support spread over the whole grid."""
    rng = np.random.default_rng(seed)
    w, h, d = size
    z_stride = h if z_stride is None else z_stride
    side = 1 << subsampling
    leaves = [(i, j, k) for k in range(z_first >> subsampling, ((z_first + d - 1) >> subsampling) + 1)
              for j in range(((h - 1) >> subsampling) + 1) for i in range(((w - 1) >> subsampling) + 1)]
    n_shared = 20
    n = n_shared + per_leaf * len(leaves)
    splats = np.zeros(n, ob.SPLAT_DTYPE)
    lo = np.array([0, 0, z_first], np.float64)
    pos = np.empty((n, 3))
    pos[:n_shared] = lo + rng.uniform(0.0, 1.0, (n_shared, 3)) * np.array(size)
    radius = np.empty(n)
    radius[:n_shared] = rng.uniform(4.0, 7.0, n_shared)
    radius[n_shared:] = rng.uniform(2.0, 3.5, n - n_shared)
    commands = [n_shared + 1] + list(range(n_shared)) + [-1]          # the shared run, at position 0
    start = np.full(morton(*np.max(np.array(leaves), axis=0).tolist()) + 1, -1, np.int32)
    for li, leaf in enumerate(leaves):
        first = n_shared + per_leaf * li
        pos[first:first + per_leaf] = (np.array(leaf) + rng.uniform(0.0, 1.0, (per_leaf, 3))) * side
        if li % 5 == 4:
            continue                                                  # a leaf without a list
        head = len(commands)
        ids = rng.permutation(np.arange(first, first + per_leaf))
        commands += [head + 1 + per_leaf] + [int(i) for i in ids] + [0 if li % 3 == 1 else -1]
        start[morton(*leaf)] = head
    splats["position"] = (pos + np.array(offset)).astype(np.float32)
    splats["radius"] = (1.0 / (radius * radius)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    splats["normal"] = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(np.float32)
    splats["quality"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
    rows = (z_first + d - 1) * z_stride + z_bias + h + 5
    return dict(offset=offset, splats=splats, commands=np.array(commands, np.int32), start=start, subsampling=subsampling,
                size=size, image_w=w + 3, rows=rows, z_stride=z_stride, z_bias=z_bias, z_first=z_first, z_last=z_first + d - 1)


CASES = {
    "5x3x3 multiply": dict(size=(40, 24, 24), offset=(100, 200, 300)),
    "1x3x2 divide": dict(size=(8, 24, 16), offset=(3, 4, 5)),
    "3x1x2 divide": dict(size=(24, 8, 16), offset=(3, 4, 5)),
    "7x5x5 tail": dict(size=(56, 40, 40), offset=(10, 20, 30)),
    "swathe": dict(size=(16, 16, 16), offset=(50, 60, 70), z_first=8, z_stride=21, z_bias=3),
    "subsampling 4": dict(size=(32, 32, 32), offset=(0, 0, 0), subsampling=4, per_leaf=400),
    "negative offsets": dict(size=(24, 16, 16), offset=(-37, -5, -100)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return blocks_fixture(seed=1 + sorted(CASES).index(name), **CASES[name])


def swathe_of(fx, size=None):
    import mlsgpu_amd as m
    w, h, d = size or fx["size"]
    return m.Swathe(w, h, fx["z_stride"], fx["z_bias"], fx["z_first"], fx["z_first"] + d - 1)


@functools.lru_cache(maxsize=None)
def expected(name, shape, size=None):
    """The oracle's field for a case (or for its first size[0] x size[1] x size[2] corners), computed once; read-only."""
    fx = case(name)
    w, h, d = size or fx["size"]
    exp = np.full((fx["rows"], fx["image_w"]), SENTINEL, np.float32)
    ob.process_corners(exp, fx["splats"], fx["commands"], fx["start"], fx["subsampling"], fx["offset"], w, h, fx["z_stride"],
                       fx["z_bias"], fx["z_first"], fx["z_first"] + d - 1, ob.lib().orc_boundary_factor(1.0), shape)
    exp.flags.writeable = False
    return exp


class Functor:
    """An MlsFunctor on a case's lists, with the device buffers it reads kept alive."""

    def __init__(self, ctx, fx, variant, shape):
        import mlsgpu_amd as m
        self.buffers = [m.DeviceBuffer(ctx, array=fx[k]) for k in ("splats", "commands", "start")]
        self.gen = m.MlsFunctor(ctx, shape)
        self.gen.set_variant(variant)
        self.gen.set_buffers(fx["offset"], *self.buffers, fx["subsampling"])


def new_field(ctx, fx):
    import mlsgpu_amd as m
    return m.DeviceBuffer(ctx, array=np.full((fx["rows"], fx["image_w"]), SENTINEL, np.float32))


def assert_same_bits(got, exp, what):
    np.testing.assert_array_equal(got.view(np.uint32), exp.view(np.uint32), err_msg=what)


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_blocks_with_their_own_lists(ctx, name, shape):
    fx = case(name)
    exp = expected(name, shape)
    fields = {}
    for variant in (5, 1):
        f = Functor(ctx, fx, variant, shape)
        field = new_field(ctx, fx)
        f.gen.enqueue(field, fx["image_w"], fx["rows"], swathe_of(fx))
        ctx.synchronize()
        fields[variant] = field.download(np.float32).reshape(fx["rows"], fx["image_w"])
    # the fixture does what it is for: blocks without a list, blocks with one, and the field depends on the block
    w, h, _ = fx["size"]
    rows = np.arange(fx["z_first"], fx["z_last"] + 1)[:, None] * fx["z_stride"] + fx["z_bias"] + np.arange(h)[None, :]
    inside = exp[rows.ravel(), :w]
    assert np.isnan(inside).any() and (~np.isnan(inside)).sum() > 200
    assert np.all(np.delete(exp, rows.ravel(), axis=0) == SENTINEL) and np.all(exp[:, w:] == SENTINEL)
    assert_same_bits(fields[5], exp, "variant 5 against the oracle")
    assert_same_bits(fields[1], exp, "variant 1 against the oracle")
    assert_same_bits(fields[5], fields[1], "variant 5 against variant 1")


def test_the_lists_tell_the_blocks_apart():
    """What the cases rest on: with the lists of two leaves exchanged the oracle's field changes, so a workgroup that reads
    another block's descriptor cannot pass."""
    fx = dict(case("5x3x3 multiply"))
    listed = np.flatnonzero(fx["start"] >= 0)
    swapped = fx["start"].copy()
    swapped[listed[0]], swapped[listed[1]] = fx["start"][listed[1]], fx["start"][listed[0]]
    w, h, d = fx["size"]
    other = np.full((fx["rows"], fx["image_w"]), SENTINEL, np.float32)
    ob.process_corners(other, fx["splats"], fx["commands"], swapped, fx["subsampling"], fx["offset"], w, h, fx["z_stride"],
                       fx["z_bias"], fx["z_first"], fx["z_last"], ob.lib().orc_boundary_factor(1.0), 0)
    assert not np.array_equal(other.view(np.uint32), expected("5x3x3 multiply", 0).view(np.uint32))


@pytest.mark.parametrize("shape", [0, 1])
def test_two_functors_in_one_launch(ctx, shape):
    """mlsgpu_hip_mls_enqueue_batch with 175 and 6 blocks: the short lane's surplus workgroups touch nothing, and each lane reads
    its own part of the descriptor table."""
    import mlsgpu_amd as m
    names = ("7x5x5 tail", "1x3x2 divide")
    for variant in (5, 1):
        functors = [Functor(ctx, case(n), variant, shape) for n in names]
        fields = [new_field(ctx, case(n)) for n in names]
        handles = (C.c_void_p * 2)(*[f.gen.h for f in functors])
        ptrs = (C.c_void_p * 2)(*[f.ptr for f in fields])
        pitches = (C.c_uint64 * 2)(*[case(n)["image_w"] for n in names])
        rows = (C.c_uint64 * 2)(*[case(n)["rows"] for n in names])
        swathes = (m.Swathe * 2)(*[swathe_of(case(n)) for n in names])
        m.binding.check(m.lib().mlsgpu_hip_mls_enqueue_batch(handles, ptrs, pitches, rows, swathes, 2))
        ctx.synchronize()
        for n, field in zip(names, fields):
            fx = case(n)
            got = field.download(np.float32).reshape(fx["rows"], fx["image_w"])
            assert_same_bits(got, expected(n, shape), "%s, variant %d" % (n, variant))


def test_small_large_small_without_synchronising(ctx):
    """One functor, three launches back to back on the stream: 4 blocks, then 175 (the descriptor table grows while the first
    launch may still read the old one), then 12 (the grown table is reused)."""
    name = "7x5x5 tail"
    fx = case(name)
    sizes = [(16, 16, 8), fx["size"], (24, 16, 16)]
    for variant in (5, 1):
        f = Functor(ctx, fx, variant, 0)
        fields = [new_field(ctx, fx) for _ in sizes]
        for size, field in zip(sizes, fields):
            f.gen.enqueue(field, fx["image_w"], fx["rows"], swathe_of(fx, size))
        ctx.synchronize()
        for size, field in zip(sizes, fields):
            got = field.download(np.float32).reshape(fx["rows"], fx["image_w"])
            exp = expected(name, 0, None if size == fx["size"] else size)
            assert_same_bits(got, exp, "%s, variant %d" % (size, variant))
