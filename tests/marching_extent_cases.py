"""Fields, shapes and memory settings of the marching extent tests (test_marching_extents_oracle.py on the CPU,
test_gpu_marching_extents.py on the device): rows of up to 8189 corners, 2049 rows a layer, 1031 slices a bucket.

Write W for corners per row, cw = W - 1 for cells and nw = ceil((2 W - 1) / 64) for the 64-bit words of a lattice row.  The
widths are the ones at which a marching kernel changes what it does (WIDTHS below gives the reason for each); the two fields
are one that the triangle-route rule sends by rows (hash noise, over three quarters of the cells occupied) and one that it
sends by cells (a tube, an eighth).  The oracle's run of a case is computed once and shared (oracle_run)."""
import functools
import time

import numpy as np

import oracle_binding as ob
from test_oracle_marching import host_generator

ALIGNMENT = (8, 8, 8)
KEY_OFFSET = (7, 0, 3)
COUNTERS = ("shipouts", "overflows", "occupied", "unwelded", "indices", "welded", "external")
MAX_CELL_BYTES = 872


def noise_fn(seed, hole_rate):
    """A hash-noise field with NaN holes: every cube code, every lattice word boundary, cells dropped by isValid."""
    def fn(x, y, z):
        h = (x.astype(np.uint64) * np.uint64(73856093)) ^ (y.astype(np.uint64) * np.uint64(19349663)) \
            ^ (np.uint64(z) * np.uint64(83492791)) ^ np.uint64(seed * 2654435761)
        h = (h * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
        v = (h.astype(np.float64) / float(1 << 24) - 0.5).astype(np.float32)
        v = np.where(v == 0, np.float32(0.25), v)
        holes = ((h >> np.uint64(7)) % np.uint64(1000)) < np.uint64(int(hole_rate * 1000))
        return np.where(holes, np.float32(np.nan), v)
    return fn


def tube_fn(axis=0):
    """A tube along `axis` whose radius swells and shrinks: with (a, b) the other two coordinates in x, y, z order and t the
    one along the axis, negative inside sqrt((a - 8.3)^2 + (b - 6.1)^2) < 2.7 + 0.8 sin(0.37 t).  Along x on W x 17 x 13."""
    def fn(x, y, z):
        c = [x.astype(np.float64), y.astype(np.float64), np.full(x.shape, float(z))]
        t = c.pop(axis)
        return (np.sqrt((c[0] - 8.3) ** 2 + (c[1] - 6.1) ** 2) - (2.7 + 0.8 * np.sin(0.37 * t))).astype(np.float32)
    return fn


def positive_fn(x, y, z):
    return np.ones(x.shape, np.float32)


FIELDS = {"noise": noise_fn(205, 0.03), "tube": tube_fn(0), "tube_y": tube_fn(1), "tube_z": tube_fn(2), "positive": positive_fn}
DENSE = {"noise": True, "tube": False, "tube_y": False, "tube_z": False}     # at least a quarter of the cells occupied: by rows


def lattice_words(width):
    return (2 * width - 1 + 63) // 64


# corners per row: the reason
WIDTHS = {
    32: "nw 1", 33: "nw 2",
    96: "nw 3",
    129: "cw 128", 130: "cw 129",
    193: "cw 192, nw 7: one round of cellCodeKernel, three chunks", 194: "cw 193: a second round, a fourth chunk",
    385: "cw 384", 386: "cw 385: a third round",
    449: "nw 15: 135 staged words, the first beyond 128", 480: "nw 15, its last word full",
    672: "nw 21: three rows a wave, one lane idle", 673: "nw 22: two rows a wave, twenty lanes idle",
    1024: "nw 32: two rows a wave", 1025: "nw 33: one row a wave from here",
    2016: "nw 63", 2017: "nw 64: every lane a word",
    2048: "nw 64: the word kernel's last width", 2049: "nw 65: the wave-per-row kernel's first, cells route forced",
    4100: "nw 129",
    8189: "nw 256: maxWidth 8192, the limit of the API",
}
NW_REQUIRED = (1, 2, 3, 7, 15, 21, 22, 32, 33, 63, 64, 65, 129)
REGIME_WIDTHS = (194, 449, 1025, 2048, 2049)
SIDES = {"noise": (9, 10), "tube": (17, 13)}             # height and depth next to the width


class Case:
    """One bucket: a field on `size` corners, marched by an object of `dims` maximum corners (the size plus 3, 2 and at least
    5, the depth a multiple of 8) and `swathe` maximum slices a swathe.  The object works in swathes of min(swathe, maxDepth)
    rounded DOWN to the z alignment: a bucket that fits one takes the lattice weld, any other the sort weld, whose buffers
    exist only when that figure is below maxDepth.  `swathes` is how many the case is meant to take, checked here."""

    def __init__(self, name, field, size, swathe=24, max_depth=None, swathes=1, fn=None):
        self.name, self.field, self.size, self.swathe = name, field, tuple(size), swathe
        self.dims = (size[0] + 3, size[1] + 2, max_depth or (size[2] + 5 + 7) // 8 * 8)
        self.fn = fn or FIELDS[field]
        self.max_swathe = min(swathe, self.dims[2]) // ALIGNMENT[2] * ALIGNMENT[2]
        self.sort_buffers = self.max_swathe < self.dims[2]
        assert -(-size[2] // self.max_swathe) == swathes, (name, self.max_swathe, swathes)
        assert swathes == 1 or self.sort_buffers

    def __repr__(self):
        return self.name

    @property
    def cells(self):
        return (self.size[0] - 1) * (self.size[1] - 1) * (self.size[2] - 1)

    def memory(self, which):
        """ "ample": the cells of a slice times maxDepth, enough for the volume and no more (the 400 slices used elsewhere
        are gigabytes at these widths); "tight": two slices, at which every case overflows and is split but those that
        the space of a single slice already holds (the tube on W x 17 x 13: test_marching_extents_oracle.py); "floor": one
        slice, the least the constructor accepts (marching_key_cases.py)."""
        slices = {"ample": self.dims[2], "tight": 2, "floor": 1}[which]
        return (self.dims[0] - 1) * (self.dims[1] - 1) * MAX_CELL_BYTES * slices


def width_case(field, width, sort_buffers=False):
    """W x 9 x 10 of noise or W x 17 x 13 of the tube in one swathe; with sort_buffers maxDepth is 32 > maxSwathe 24, which
    keeps the sort weld's buffers (the lattice weld is still the one chosen: the depth fits a swathe)."""
    h, d = SIDES[field]
    case = Case("%s%d%s" % (field, width, "s" if sort_buffers else ""), field, (width, h, d), 24, 32 if sort_buffers else 24)
    assert case.sort_buffers == sort_buffers
    return case


EXTENT_CASES = [
    Case("tall1031", "noise", (11, 1031, 13)),                       # 2061 lattice rows a layer
    Case("tall2049", "noise", (9, 2049, 10)),                        # 4097
    Case("tall_tube", "tube_y", (17, 1031, 13)),
    Case("deep_swathes", "noise", (11, 13, 1031), swathe=64, swathes=17),        # 17 swathes: sort weld, copy_slice between every pair
    Case("deep_one", "noise", (11, 13, 1031), swathe=1040),          # one swathe of 1031 slices: lattice weld
    Case("deep_tube_swathes", "tube_z", (17, 13, 1031), swathe=64, swathes=17),
    Case("deep_tube_one", "tube_z", (17, 13, 1031), swathe=1040),
    Case("wide_swathes", "noise", (2049, 9, 40), swathe=16, swathes=3),         # nw 65 over three swathes
]

# thin grids for the per-vertex float64 checker, each with both fields
THIN_SIZES = [(2049, 5, 4), (4100, 5, 4), (8189, 4, 4), (5, 2049, 4), (5, 4, 2049)]


@functools.lru_cache(maxsize=None)
def thin_tube_fn(axis):
    """The tube scaled into a thin grid: on sides of 4 or 5 corners the tube of FIELDS would miss the section altogether."""
    def fn(x, y, z):
        c = [x.astype(np.float64), y.astype(np.float64), np.full(x.shape, float(z))]
        t = c.pop(axis)
        return (np.sqrt((c[0] - 1.9) ** 2 + (c[1] - 1.4) ** 2) - (1.1 + 0.4 * np.sin(0.37 * t))).astype(np.float32)
    return fn


def thin_case(field, size):
    """A thin grid of noise or of the scaled tube along its long side, in one swathe."""
    fn = FIELDS["noise"] if field == "noise" else thin_tube_fn(int(np.argmax(size)))
    return Case("%s_%dx%dx%d" % ((field,) + tuple(size)), field, size, swathe=(size[2] + 5 + 7) // 8 * 8, fn=fn)


# mixed batches: lanes of different maximum sizes in one generate_batch call
BATCH_A = [Case("a_noise2048", "noise", (2048, 9, 10)),              # rows route, nw 64
           Case("a_noise97", "noise", (97, 35, 13)),                 # rows route, nw 4
           Case("a_tube1025", "tube", (1025, 17, 13)),               # cells route
           Case("a_positive", "positive", (33, 9, 9))]               # no surface: no ship-out
BATCH_B = BATCH_A + [Case("b_noise2049", "noise", (2049, 9, 10))]    # nw 65: the wave-per-row mask kernel for every lane
BATCHES = {"a": BATCH_A, "b": BATCH_B,
           "a_reversed": BATCH_A[::-1]}                              # the narrow rows-route lane ahead of the wide one


ORACLE_SECONDS = {}          # the arguments of _oracle_run: what the run took


@functools.lru_cache(maxsize=None)
def _oracle_run(fn, size, dims, swathe, mesh_memory, key_offset):
    t = time.perf_counter()
    oracle = ob.MarchingOracle(dims[0], dims[1], dims[2], swathe, mesh_memory, ALIGNMENT)
    batches = oracle.generate(host_generator(fn), size, key_offset)
    ORACLE_SECONDS[fn, size, dims, swathe, mesh_memory, key_offset] = time.perf_counter() - t
    for b in batches:
        for a in b.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return batches, oracle.stats()


def oracle_run(case, memory, key_offset=KEY_OFFSET):
    """(batches, stats) of the oracle on a case with "ample", "tight" or "floor" mesh memory; computed once, read-only."""
    return _oracle_run(case.fn, case.size, case.dims, case.swathe, case.memory(memory), tuple(key_offset))


def oracle_seconds(case, memory, key_offset=KEY_OFFSET):
    """What that run took when it was made (not a later look into the cache)"""
    oracle_run(case, memory, key_offset)
    return ORACLE_SECONDS[case.fn, case.size, case.dims, case.swathe, case.memory(memory), tuple(key_offset)]


def field_array(fn, size):
    """The field [z, y, x] a generator function gives, as marching_fp64 takes it."""
    W, H, D = size
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    return np.stack([np.asarray(fn(xs, ys, z), np.float32) for z in range(D)])
