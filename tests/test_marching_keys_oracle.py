"""The marching key cases (tests/marching_key_cases.py) on the CPU: the conditions under which a case puts the sort weld where
it was chosen to -- 31, 32, 33 or 34 bits of compact key, several ship-outs inside a bucket, keys beyond 2^32 -- asserted,
not merely reported, from the oracle's batches and stats.  test_gpu_marching_keys.py holds the kernels to the same runs."""
import ctypes as C

import numpy as np
import pytest

import marching_extent_cases as mx
import marching_key_cases as mk

KEY_AXIS_BITS = 21
GIB = 1 << 30


def test_layouts():
    """bits = bitsFor(2 (W - 1)) + bitsFor(2 (H - 1)) + bitsFor(2 (D - 1)) + 1 as beginGenerate computes it is the table's
    column; 32-bit keys up to 32, 64-bit keys above; every step from 31 to 34 occurs."""
    assert [mk.bits_for(v) for v in (0, 1, 2, 3, 4, 1023, 1024, 2047, 2048, 2064)] == [1, 1, 2, 2, 3, 10, 11, 11, 12, 12]
    for name in mk.NAMES:
        size, bits = mk.GRIDS[name][:2]
        assert mk.key_bits(size) == bits, name
        assert (bits > 32) == (name in mk.WIDE)
        for route in ("swathes", "one", "forced"):
            if (name, route) in mk.ROUTES:
                assert mk.key_bits(mk.case(name, route).size) == bits
    assert {mk.GRIDS[n][1] for n in mk.NAMES} == {31, 32, 33, 34}
    assert [n for n in mk.NAMES if mk.GRIDS[n][1] <= 32] == ["k31", "k32_a", "k32_b"]
    assert mk.layout(mk.GRIDS["k32_a"][0]) == (11, 11, 9) and mk.layout(mk.GRIDS["k32_b"][0]) == (10, 11, 10)
    assert sum(mk.layout(mk.GRIDS["k33_deep"][0])[:2]) == 20              # the z field ends at bit 31
    assert mx.lattice_words(mk.GRIDS["k33_wide"][0][0]) == 65
    assert [mk.sort_launches(mk.GRIDS[n][0]) for n in mk.NAMES] == [12] * 7         # four passes: 8, 8, 8 and 9, 9 bits


def decode(keys, key_offset=mx.KEY_OFFSET):
    """(x2, y2, z2) of output keys with the key offset taken off, by the shifts of packedKeyOffset"""
    off = (key_offset[2] << (2 * KEY_AXIS_BITS + 1)) | (key_offset[1] << (KEY_AXIS_BITS + 1)) | (key_offset[0] << 1)
    k = keys.astype(np.uint64) - np.uint64(off)
    m = np.uint64((1 << KEY_AXIS_BITS) - 1)
    return k & m, (k >> np.uint64(KEY_AXIS_BITS)) & m, k >> np.uint64(2 * KEY_AXIS_BITS)


def compact_keys(x2, y2, z2, flag, L):
    bx, by, bz = L
    return (flag.astype(np.uint64) << np.uint64(bx + by + bz)) | (z2 << np.uint64(bx + by)) | (y2 << np.uint64(bx)) | x2


@pytest.mark.parametrize("name", mk.NAMES)
def test_swathes_route_conditions(name):
    size, bits, swathe, _, _ = mk.GRIDS[name]
    case = mk.case(name, "swathes")
    assert case.sort_buffers and case.max_swathe == swathe < size[2]      # Case has checked the number of swathes
    batches, st = mk.oracle_run(case)
    print("%s: %d x %d x %d, %d bits, oracle %.2f s, %d swathes, %d ship-outs, %d overflows, %d welded, %d external"
          % ((case.name,) + size + (bits, mk.oracle_seconds(case), -(-size[2] // swathe), st["shipouts"],
                                    st["overflows"], st["welded"], st["external"])))
    assert len(batches) == st["shipouts"] >= 1
    if name in mk.MANY_SHIPOUTS:
        assert st["shipouts"] >= 3            # z2 >= zMax2 decides externality in the middle of the bucket, not the flag alone
    internal = sum(b["num_internal"] for b in batches)
    assert internal >= 1000 and st["external"] >= 1000 and internal + st["external"] == st["welded"]

    L = mk.layout(size)
    x2, y2, z2 = (np.concatenate(a) for a in zip(*[decode(b["keys"][b["num_internal"]:]) for b in batches]))
    top = [2 * (n - 1) for n in size]
    for axis, (v, t) in enumerate(zip((x2, y2, z2), top)):
        assert int(v.min()) == 0 and int(v.max()) == t, (name, axis)
    # the compact keys as generateElements packs them: the flag it sets itself is that of the x and y faces (z comes from the
    # ship-out's bounds), and there are vertices of both kinds among the external ones
    flag = (x2 == 0) | (y2 == 0) | (x2 == top[0]) | (y2 == top[1])
    assert int(flag.sum()) >= 1000 and int((~flag).sum()) >= 100
    compact = compact_keys(x2, y2, z2, flag, L)
    assert int(compact.max()) < 1 << bits
    assert (int(compact.max()) >= 1 << 32) == (bits > 32)

    if name in mk.HIGH_Z:
        assert size[2] - 1 > 1 << (L[2] - 2)                              # slices beyond the one at which the top z bit begins
        high = high_z_internal(batches, L[2])
        print("%s: %d internal vertices with bit %d set" % (case.name, high, sum(L) - 1))
        assert high >= 1000
        assert (sum(L) - 1 >= 32) == (name == "k34")                      # k34: internal compact keys >= 2^32
        assert sum(L) - 1 >= 31


def high_z_internal(batches, bz, key_offset=mx.KEY_OFFSET):
    """Internal vertices with the top bit of the z field set, bit bx + by + bz - 1 of the compact key.  Internal vertices carry
    no key in the output, so from the positions, which include the key offset: a vertex of local cell slice cz has z2 = 2 cz
    or 2 cz + 1, and z2 >= 2^(bz - 1) iff floor(z) - offset >= 2^(bz - 2)."""
    return sum(int((np.floor(b["vertices"][:b["num_internal"], 2]) - key_offset[2] >= 1 << (bz - 2)).sum()) for b in batches)


def test_top_z_bit_needs_more_than_a_power_of_two_slices():
    """Why the deep grids are 1033 slices: k33_deep's field on 2^10 + 1 = 1025, the cheapest depth with 12 bits, has the top bit
    of the z field at the last corner alone, z2 = 2048 = 2 zMax of the last ship-out, where every vertex is external -- no
    internal vertex carries it.  The positions do include the key offset: the lowest is at z = KEY_OFFSET[2]."""
    size, c = (257, 257, 1025), mk.GRIDS["k33_deep"][3]
    assert mk.layout(size) == mk.layout(mk.GRIDS["k33_deep"][0]) and size[2] - 1 == 1 << (mk.layout(size)[2] - 2)
    case = mx.Case("k33_deep_1025", "corner", size, swathe=64, swathes=17, fn=mk.corner_fn(size, c))
    batches, st = mk.oracle_run(case)
    assert sum(b["num_internal"] for b in batches) >= 1000
    assert min(float(b["vertices"][:, 2].min()) for b in batches) == mx.KEY_OFFSET[2]
    assert max(float(b["vertices"][:, 2].max()) for b in batches) == mx.KEY_OFFSET[2] + size[2] - 1
    assert high_z_internal(batches, mk.layout(size)[2]) == 0


@pytest.mark.parametrize("name", mk.FORCED)
def test_forced_route_conditions(name):
    """One swathe and a mesh that the floor holds: a single ship-out, so MLSGPU_HIP_WELD=sort sorts the bucket at once."""
    case = mk.case(name, "forced")
    _, st = mk.oracle_run(case)
    space = (case.dims[0] - 1) * (case.dims[1] - 1) * 13
    print("%s: oracle %.2f s, %d unwelded vertices of %d" % (case.name, mk.oracle_seconds(case), st["unwelded"],
                                                            space))
    assert st["shipouts"] == 1 and st["overflows"] == 0
    assert space // 2 < st["unwelded"] <= space             # and no small one: the sort's n is most of what the buffers hold


@pytest.mark.parametrize("name,route", mk.ROUTES, ids=lambda v: v)
def test_device_memory_below_8_gib(name, route):
    """What mlsgpu_hip_marching_create would allocate for the case (host side of the library only, no GPU): a condition of
    a test on a shared machine."""
    import mlsgpu_amd
    case = mk.case(name, route)
    usage = mlsgpu_amd.lib().mlsgpu_hip_marching_resource_usage(case.dims[0], case.dims[1], case.dims[2], case.swathe,
                                                                case.memory(mk.MEMORY), (C.c_uint32 * 3)(*mx.ALIGNMENT))
    print("%s: %.2f GiB" % (case.name, usage / GIB))
    assert case.memory(mk.MEMORY) == (case.dims[0] - 1) * (case.dims[1] - 1) * mx.MAX_CELL_BYTES
    assert 0 < usage < 8 * GIB
