"""The marching sequence cases (tests/marching_sequence_cases.py) on the CPU: the conditions under which a sequence on one
object can tell a kernel that reads stale state from one that does not, so that test_gpu_marching_sequences.py cannot pass
vacuously.

Asserted, not merely reported: every step takes the weld, the triangle route, the number of swathes and the overflow (or none)
that it states; every step with a surface has more than 100 triangles and the positive one none; between two steps the earlier
one leaves a SURFACE where the later one does not reach (or the pair says why that is void); the oracle itself depends neither
on the object's dims nor on padding; the poisoning generators' blocks hold the field where it belongs and poison elsewhere."""
import functools

import numpy as np
import pytest

import marching_extent_cases as mx
import marching_key_cases as mk
import marching_sequence_cases as ms
from refdata import canonical_mesh

STEP_SETS = ["wide", "deep", "keys", "padded"]          # wide_reversed has wide's steps


def check_step(obj, step, memory):
    """What a step states against the oracle's run of it on a fresh object of the sequence's dims"""
    batches, st = ms.oracle_step(obj, step, memory)
    print("%s/%s %s: %d x %d x %d, oracle %.2f s, occupied %.3f, %d triangles, %d ship-outs, %d overflows"
          % ((obj.name, step.name, memory) + step.size + (ms.oracle_step_seconds(obj, step, memory), st["occupied"] / step.cells,
                                                         st["indices"] // 3, st["shipouts"], st["overflows"])))
    assert all(n <= m for n, m in zip(step.size, obj.dims))
    assert -(-step.size[2] // obj.max_swathe) == step.swathes, step
    one_swathe = step.size[2] <= obj.max_swathe
    if step.force_sort:
        assert one_swathe and obj.sort_buffers, step                        # the setting has something to force, and can
    assert step.weld == ("lattice" if one_swathe and not step.force_sort else "sort"), step
    assert step.weld == "lattice" or obj.sort_buffers, step
    assert (st["overflows"] > 0) == (memory in step.overflows), (step, memory, st["overflows"])
    if not step.surface:
        assert batches == [] and not any(st.values()) and step.route is None
        return st
    assert st["indices"] > 3 * 100 and len(batches) == st["shipouts"] >= 1
    if memory != "tight":
        # the route rule of a lattice ship-out: cells from nw 65 or under a quarter of the cells occupied
        if step.weld == "lattice":
            cells_route = mx.lattice_words(step.size[0]) > 64 or st["occupied"] * 4 < step.cells
            assert step.route == ("cells" if cells_route else "rows"), (step, st["occupied"] / step.cells)
        else:
            assert step.route is None
    else:
        ample = ms.oracle_step(obj, step, "ample")[1]
        assert st["indices"] == ample["indices"] and st["occupied"] == ample["occupied"]
        assert (st["shipouts"] > ample["shipouts"]) == ("tight" in step.overflows)
    return st


@pytest.mark.parametrize("name", STEP_SETS)
def test_steps_take_what_they_state(name):
    obj, steps = ms.SEQUENCES[name]
    for memory in ms.MEMORIES[name]:
        for step in dict.fromkeys(steps):
            check_step(obj, step, memory)


def test_failure_and_batch_steps():
    """The 3-swathe bucket whose generator fails, with a ship-out before its second swathe at tight memory (swathe one
    overflows), and the lanes of the rotated batches with their own key offsets."""
    for memory in ("ample", "tight"):
        st = check_step(ms.DEEP, ms.FAILING, memory)
        for rotation in range(3):
            for step in ms.batch_call(rotation):
                check_step(ms.WIDE, step, memory)
    assert st["overflows"] >= 3
    assert len({s.key_offset for s in ms.batch_call(0)}) == 3
    for k in range(3):
        assert len({ms.batch_call(r)[k].size for r in range(3)}) == 3        # a lane sees all three sizes
    for size in ms.BEYOND:
        assert sorted(np.subtract(size, ms.DEEP.dims)) == [0, 0, 1]


def test_the_thresholds_are_reached():
    """The widths, the equalities and the key widths the sequences were chosen for"""
    assert [mx.lattice_words(s.size[0]) for s in ms.WIDE_STEPS] == [65, 1, 65, 2, 33, 64, 15, 1]
    assert ms.WIDE_STEPS[0].size == ms.WIDE.dims and ms.DEEP_STEPS[4].size == ms.DEEP.dims      # size == dims, every axis
    assert ms.WIDE.max_swathe == ms.WIDE.dims[2] and not ms.WIDE.sort_buffers        # w_full: the most lattice rows there are
    assert mx.lattice_words(ms.WIDE_STEPS[0].size[0]) == mx.lattice_words(ms.WIDE.dims[0])      # L.nw == latWords
    assert ms.DEEP.max_swathe == 64 and ms.DEEP.sort_buffers
    assert ms.DEEP_STEPS[1].size[2] == ms.DEEP.max_swathe and ms.DEEP_STEPS[2].size[2] == ms.DEEP.max_swathe + 1
    assert ms.DEEP_STEPS[6].size == ms.DEEP_STEPS[1].size and ms.DEEP_STEPS[5].weld == "lattice"
    assert [mk.key_bits(s.size) for s in ms.KEYS_STEPS] == [32, 34, 22, 34, 32]
    assert (ms.PADDED.pitch, ms.PADDED.z_stride) == (2056, 24) and (ms.WIDE.pitch, ms.WIDE.z_stride) == (2056, 24)
    assert (ms.DEEP.pitch, ms.DEEP.z_stride) == (72, 40)
    for obj in (ms.WIDE, ms.DEEP, ms.KEYS, ms.PADDED):
        assert (obj.max_swathe + 1) * obj.z_stride <= obj.field_rows              # a swathe's blocks lie inside the image


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------

SLAB = 72           # slices of a slab of a deep field


@functools.lru_cache(maxsize=None)
def stale_surface(fn, size, later):
    """sign_changes_outside of the field (fn, size) against a later step's size; fields deeper than two slabs are sampled in
    their first and last SLAB slices (a lower bound, which is all the condition needs)."""
    W, H, D = size
    slabs = [(0, D)] if D <= 2 * SLAB else [(0, SLAB), (D - SLAB, D)]
    total = None
    for z0, z1 in slabs:
        ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
        field = np.stack([np.asarray(fn(xs, ys, z), np.float32) for z in range(z0, z1)])
        shifted = (later[0], later[1], max(later[2] - z0, 0))
        n = ms.sign_changes_outside(field, shifted)
        if n is not None:
            total = (total or 0) + n
    return total


def pair_condition(steps, i):
    """(count, what) for the pair (i - 1, i): the sign changes the earlier step's field has where the later one does not
    reach; None where the earlier one is larger in no axis.  An earlier step WITHOUT a surface (the positive one) hides
    nothing and overwrites only its own extent: the image beyond both still holds the step before it, which is then the one
    judged, in the region neither of the two covers."""
    later = steps[i].size
    j = i - 1
    while j >= 0 and not steps[j].surface:
        later = tuple(max(a, b) for a, b in zip(later, steps[j].size))
        j -= 1
    if j < 0:
        return None, "nothing with a surface before"
    n = stale_surface(steps[j].fn, steps[j].size, later)
    return n, "%s beyond %d x %d x %d" % ((steps[j].name,) + later)


# the pairs whose condition is void (the earlier step, or the one judged in its place, is larger in no axis), by the name of
# the LATER step; every other pair must leave a surface behind
VOID = {
    "wide": {"w_tube2049",       # after 32 x 17 x 13
             "w_nw33"},          # after 33 x 5 x 4 (w_nw64 after 1025 x 20 x 13 is not: rows 17 to 19 stay behind)
    "wide_reversed": {"w_positive",                     # after 32 x 17 x 13
                      "w_nw64",                         # after the positive step, behind which 32 x 17 x 13 is judged
                      "w_tube2049", "w_full"},          # after 33 x 5 x 4 and 32 x 17 x 13
    "deep": {"d_full_tube", "d_64_forced"},             # after 65 x 33 x 2 and 33 x 33 x 40
    "keys": {"k34"},             # after k_small; after k32_clipped it is not void: 260 > 257 corners in x
    "padded": set(),
}


@pytest.mark.parametrize("name", sorted(ms.SEQUENCES))
def test_earlier_step_leaves_a_surface_where_the_later_does_not_reach(name):
    """Per pair, printed: the stale surface a kernel reading past the current width, row, slice or record count would find.
    A pair is void only if the earlier step is larger in no axis; the names of the void pairs' later steps are stated in
    VOID and the rest asserted to have sign changes."""
    _, steps = ms.SEQUENCES[name]
    void = set()
    for i in range(1, len(steps)):
        n, what = pair_condition(steps, i)
        print("%s: %s -> %s: %s: %s" % (name, steps[i - 1].name, steps[i].name, what, "void" if n is None else "%d sign changes" % n))
        if n is None:
            void.add(steps[i].name)
        else:
            assert n > 0, (name, steps[i - 1].name, steps[i].name)
    assert void == VOID[name], (name, sorted(void))
    assert len(void) < len(steps) - 1


# ---- the oracle is history-free and padding-free ------------------------------------------------------------------------------

def test_oracle_depends_neither_on_dims_nor_on_padding():
    """Step 2 of the wide sequence on a fresh oracle object of dims 35 x 19 x 24 and on one of 2052 x 20 x 24: the same
    welded vertices and triangles (the oracle's generator writes no padding, and every oracle_step is a fresh object, so
    there is no history either).  Batch boundaries follow the mesh memory, which follows the dims: at two slices of
    34 x 18 cells (15 912 vertices) the bucket's 56 k vertices overflow and come in several batches, at two slices of
    2051 x 19 cells in one; with ample memory both give one."""
    step = ms.WIDE_STEPS[1]
    small = ms.Obj("small", (35, 19, 24), 24)
    ref = None
    counts = {}
    for obj in (small, ms.WIDE):
        for memory in ("ample", "tight"):
            batches, st = ms.oracle_step(obj, step, memory)
            print("%s %s: oracle %.2f s, %d batches" % (obj.name, memory, ms.oracle_step_seconds(obj, step, memory), len(batches)))
            counts[obj.name, memory] = len(batches)
            got = canonical_mesh(batches)
            if ref is None:
                ref = got
                assert len(ref[1]) > 100
            else:
                np.testing.assert_array_equal(ref[0].view(np.uint32), got[0].view(np.uint32))
                np.testing.assert_array_equal(ref[1], got[1])
    assert counts["small", "ample"] == counts["wide", "ample"] == counts["wide", "tight"] == 1
    assert counts["small", "tight"] > 1
    # with equal batch boundaries the batches themselves are equal, keys and all
    a, b = ms.oracle_step(small, step, "ample")[0], ms.oracle_step(ms.WIDE, step, "ample")[0]
    for k in ("vertices", "triangles", "keys"):
        np.testing.assert_array_equal(a[0][k].view(np.uint32 if k == "vertices" else a[0][k].dtype), b[0][k].view(
            np.uint32 if k == "vertices" else b[0][k].dtype))
    assert a[0]["num_internal"] == b[0]["num_internal"]


# ---- the poisoned blocks, on the host arrays ------------------------------------------------------------------------------------

def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("poison", ms.POISONS)
def test_poison_blocks(poison):
    """The field bit for bit in [0, height) x [0, width); elsewhere NaN, or +-3e38 whose sign flips between any two
    neighbours (in the next slice too), or the field function beyond the extent -- and with the first two no field value at
    all out there."""
    for obj, step in [(ms.WIDE, ms.WIDE_STEPS[1]), (ms.WIDE, ms.WIDE_STEPS[2]), (ms.WIDE, ms.WIDE_STEPS[0]),
                      (ms.DEEP, ms.DEEP_STEPS[2]), (ms.DEEP, ms.DEEP_STEPS[5]), (ms.PADDED, ms.PADDED_STEPS[1])]:
        W, H, D = step.size
        field = mx.field_array(step.fn, step.size)
        for z in sorted({0, 1, D - 1}):
            block = ms.poison_block(step.fn, poison, z, W, H, obj.z_stride, obj.pitch)
            assert block.shape == (obj.z_stride, obj.pitch) and block.dtype == np.float32
            assert same_bits(block[:H, :W], field[z])
            outside = np.ones(block.shape, bool)
            outside[:H, :W] = False
            assert outside.any() == (step.size[:2] != (obj.pitch, obj.z_stride))
            out = block[outside]
            if poison == "nan":
                assert np.isnan(out).all()
            elif poison == "big":
                ys, xs = np.nonzero(outside)
                assert np.array_equal(out, np.where((xs + ys + z) & 1, np.float32(-3e38), np.float32(3e38)))
                nxt = ms.poison_block(step.fn, poison, z + 1, W, H, obj.z_stride, obj.pitch)
                assert np.all(np.sign(nxt[outside]) == -np.sign(out))
                both = outside[:, 1:] & outside[:, :-1]
                assert np.all((np.sign(block[:, 1:]) == -np.sign(block[:, :-1]))[both])
                both = outside[1:] & outside[:-1]
                assert np.all((np.sign(block[1:]) == -np.sign(block[:-1]))[both])
            else:
                ys, xs = np.meshgrid(np.arange(obj.z_stride, dtype=np.uint32), np.arange(obj.pitch, dtype=np.uint32), indexing="ij")
                assert same_bits(out, np.asarray(step.fn(xs, ys, z), np.float32)[outside])


# ---- the worker's buckets ------------------------------------------------------------------------------------------------------

def test_worker_buckets_have_a_surface():
    """Every bucket of the worker sequence but the one of 0 splats cuts the shells: more than 100 triangles each"""
    items = ms.worker_items(len(ms.worker_cloud()))
    for i, ((first, count, low, nv), size) in enumerate(zip(items, ms.WORKER_SIZES)):
        exp, st, seconds = ms.worker_oracle(i)
        print("%s at %s: oracle %.2f s, %d triangles" % (nv, low, seconds, st["indices"] // 3))
        if size is None:
            assert exp == [] and count == 0
        else:
            assert st["indices"] > 3 * 100
    for order in ms.WORKER_ORDERS:
        assert sorted(order[0] + order[1]) == list(range(6))
        for lane in range(3):
            assert ms.WORKER_SIZES[order[0][lane]] != ms.WORKER_SIZES[order[1][lane]]
    # ... and across the two orders, whose calls follow one another on one worker
    for lane in range(3):
        assert ms.WORKER_SIZES[ms.WORKER_ORDERS[0][1][lane]] != ms.WORKER_SIZES[ms.WORKER_ORDERS[1][0][lane]]
