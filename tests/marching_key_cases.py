"""Grids of the marching key tests (test_marching_keys_oracle.py on the CPU, test_gpu_marching_keys.py on the device): buckets
whose compact weld key takes 31 to 34 bits, on both sides of the step from 32-bit to 64-bit keys.

marching.hip packs a vertex's doubled local coordinates and its external flag into [ext][z2 : bz][y2 : by][x2 : bx] with
b = bitsFor(2 (N - 1)) per axis and sorts on bx + by + bz + 1 bits; above 32 the weld runs in its uint64_t instantiations.
The layout works in bit fields and the flag has a bit of its own, so a side of 2^(b - 2) + 1 corners is the cheapest with b
bits and 33 bits are reached at 2^26 corners -- not at (2 W)(2 H)(2 D) >= 2^32.

The field is noise in a few places and no surface elsewhere, so that a run costs the scan of the grid and not its mesh; mesh
memory is the floor the constructor accepts (one slice of maximum cells).  Every case is built for one of three routes:

swathes  a swathe well below the depth: the sort weld across several swathes, copy_slice between them
one      a swathe of the whole depth: the lattice weld, no key layout enters -- the case itself on the device
forced   one swathe covers the depth, but maxDepth > maxSwathe keeps the sort buffers: with MLSGPU_HIP_WELD=sort the whole
         bucket goes through ONE sort, the largest the sort of that key type sees"""
import functools

import numpy as np

import marching_extent_cases as mx

MEMORY = "floor"


def bits_for(max_value):
    """bitsFor of marchingplan.hpp"""
    b = 1
    while (max_value >> b) != 0:
        b += 1
    return b


def layout(size):
    """(bx, by, bz) of beginGenerate for a bucket of `size` corners"""
    return tuple(bits_for(2 * (n - 1)) for n in size)


def key_bits(size):
    return sum(layout(size)) + 1


@functools.lru_cache(maxsize=None)
def corner_fn(size, c):
    """Noise in a column of c + 1 corners square at the far x, y edge, one of 6 at the near edge and a patch of 12 x 12 under
    the top face in the middle of the slice; 1 (no surface) everywhere else."""
    W, H, D = size
    noise = mx.noise_fn(205, 0.03)

    def fn(x, y, z):
        v = noise(x, y, z)
        on = ((x >= W - 1 - c) & (y >= H - 1 - c)) | ((x < 6) & (y < 6))
        if z >= D - 4:
            on = on | ((x >= W // 2 - 6) & (x < W // 2 + 6) & (y >= H // 2 - 6) & (y < H // 2 + 6))
        return np.where(on, v, np.float32(1.0))
    return fn


# name: size, key bits, slices a swathe of route "swathes", c of the routes "swathes" and "one", c of route "forced".
# The noise gives about 9.5 unwelded vertices a cell and the floor holds 13 a cell of ONE slice.  c of "swathes": a swathe's
# share of the far column, (c + 1)^2 cells a slice, fits the floor and two or three swathes' do not, so the bucket is shipped
# out several times without an overflow (k33_wide: a single ship-out; three would take 40 M vertices).  c of "forced": the
# whole column fits the floor, nearly filling it: one ship-out, one sort of 0.87 M to 3.2 M keys.
GRIDS = {
    "k31": ((512, 512, 257), 31, 64, 70, None),               # 32-bit keys, top bit free: the control
    "k32_a": ((513, 513, 129), 32, 32, 90, None),             # 32-bit keys, flag in bit 31, sort on the whole word
    "k32_b": ((512, 513, 257), 32, 64, 70, 40),               # the same with the bits spread (10, 11, 10)
    "k33_square": ((513, 513, 257), 33, 64, 70, 40),          # 64-bit keys, only the flag above bit 31
    "k33_deep": ((257, 257, 1033), 33, 64, 20, 8),            # bx + by = 20: z bits reach bit 31; 17 swathes
    "k33_wide": ((2049, 1025, 33), 33, 16, 40, None),         # nw 65: wave-per-row mask kernel, cells route forced
    "k34": ((257, 513, 1033), 34, 64, 30, None),              # coordinates above bit 31: internal keys >= 2^32; 2^27 corners
}
# The two deep grids are 1033 slices and not 2^10 + 1 = 1025: on a side of 2^(b - 2) + 1 corners the top bit of the b-bit field
# is set at the last corner alone, 2 (D - 1) = 2^(b - 1), and every vertex there is external (z2 >= 2 zMax at the last
# ship-out).  Eight more slices put INTERNAL vertices at z2 = 2048 .. 2063, with the same bit counts and 17 swathes.
NAMES = tuple(GRIDS)
WIDE = tuple(n for n in NAMES if GRIDS[n][1] > 32)
ONE = ("k32_a", "k33_square", "k33_wide", "k34")
FORCED = ("k32_b", "k33_square", "k33_deep")
MANY_SHIPOUTS = ("k31", "k32_a", "k32_b", "k33_square", "k33_deep", "k34")        # route "swathes": at least three ship-outs
HIGH_Z = ("k33_deep", "k34")                                             # internal vertices with the top bit of z2 set


@functools.lru_cache(maxsize=None)
def case(name, route):
    size, _, swathe, c, c_forced = GRIDS[name]
    depth = (size[2] + 5 + 7) // 8 * 8
    if route == "swathes":
        k = mx.Case("%s_swathes" % name, "corner", size, swathe=swathe, swathes=-(-size[2] // swathe), fn=corner_fn(size, c))
        assert k.max_swathe == swathe
    elif route == "one":
        k = mx.Case("%s_one" % name, "corner", size, swathe=depth, fn=corner_fn(size, c))
        assert not k.sort_buffers
    else:
        assert route == "forced"
        k = mx.Case("%s_forced" % name, "corner", size, swathe=depth, max_depth=depth + 8, fn=corner_fn(size, c_forced))
        assert k.sort_buffers and k.max_swathe >= size[2]
    return k


ROUTES = [(n, "swathes") for n in NAMES] + [(n, "one") for n in ONE] + [(n, "forced") for n in FORCED]

def oracle_run(k, key_offset=mx.KEY_OFFSET):
    """mx.oracle_run at the floor"""
    return mx.oracle_run(k, MEMORY, key_offset)


def oracle_seconds(k, key_offset=mx.KEY_OFFSET):
    """What that run took when it was made, whoever made it (mx.oracle_seconds)"""
    return mx.oracle_seconds(k, MEMORY, key_offset)


def sort_launches(size):
    """Launches of one radix sort of the weld: three a pass, digits of at most 10 bits for 4-byte keys and 9 for 8-byte keys"""
    bits = key_bits(size)
    return 3 * -(-bits // (9 if bits > 32 else 10))
