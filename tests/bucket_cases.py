"""Clouds that drive the device bucketer (mlsgpu_amd/csrc/bucket.hip) where the random cases and the uniform clouds never
go: grids whose lower ends lie beyond 2^29 cells, splats of 10^9 .. 10^12 cells, splats that span more than 31 microblocks,
a whole counting span in one microblock, and boxes that no integer holds.

numpy only, seeded.  A builder returns (splats, grid, params), grid and params shaped as bucket_checks.random_case returns
them; CASES names the instances the tests run.  What each cloud is FOR is asserted by tests/test_bucket_cases.py, so that an
edit here cannot quietly stop a case from reaching its branch.
"""
import numpy as np

from oracle_binding import SPLAT_DTYPE

PRIV_SPAN = 63 * 1024           # bucket.hip: elements of one workgroup of bucketCountPrivateKernel (enum PRIV_SPAN)
PRIV_LDS_BYTES = 160 * 1024     # bucket.hip: the LDS image of that kernel may take this much
NOTE_MAX_SPAN = 31              # bucket.hip, RegionView::packNote: hi - lo per axis that a kept range holds (5 bits)
SORT_MAX_DIGIT_BITS = 10        # primitives.hpp: SortCaps<uint32_t>::MAX_DIGIT_BITS (more region bits: several sort passes)
NARROW_FIRST = 1 << 29          # bucket.hip, RegionView::rangeOf: 32-bit cell arithmetic needs |grid lower end| below this
NARROW_CELL = 1.0e9             # ... and |floored cell| below this
CLAMP = 2.0 ** 62               # rangeOf / the oracle's splatToBuckets: a box beyond 2^62 cells is taken to reach 2^62


def _splats(position, radius):
    n = len(radius)
    s = np.zeros(n, SPLAT_DTYPE)
    s["position"] = np.asarray(position, np.float64).reshape(n, 3).astype(np.float32)
    s["radius"] = np.asarray(radius, np.float64).astype(np.float32)
    s["normal"] = (1.0, 0.0, 0.0)
    s["quality"] = 1.0
    return s


def _params(max_splats, max_cells, chunk_cells, micro_cells, max_split):
    return dict(max_splats=max_splats, max_cells=max_cells, chunk_cells=chunk_cells, micro_cells=micro_cells, max_split=max_split)


def cell_box_clamped(splats, grid):
    """bucket_checks.cell_box with the floored float clipped to +-2^62 before it becomes an integer, as rangeOf and the
    oracle do: the same numbers for every box below 2^62 cells, and defined ones beyond (infinite corners included)."""
    inv = np.float32(1.0) / np.float32(grid["spacing"])
    ref = np.asarray(grid["reference"], np.float32)
    first = np.asarray(grid["extents"], np.int64).reshape(3, 2)[:, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        fl = np.floor(((splats["position"] - splats["radius"][:, None]) - ref) * inv)
        fh = np.floor(((splats["position"] + splats["radius"][:, None]) - ref) * inv)
    assert fl.dtype == np.float32 and fh.dtype == np.float32
    lo = np.clip(fl, np.float32(-CLAMP), np.float32(CLAMP)).astype(np.int64) - first
    hi = np.clip(fh, np.float32(-CLAMP), np.float32(CLAMP)).astype(np.int64) - first
    return lo, hi


def micro_range(splats, grid, micro):
    """(lo, hi, meets): every splat's microblock range on the grid's top level without chunks, clamped as
    BucketState::clamp does, and whether it is non-empty."""
    ext = np.asarray(grid["extents"], np.int64).reshape(3, 2)
    dims = (ext[:, 1] - ext[:, 0] + micro - 1) // micro
    lo, hi = cell_box_clamped(splats, grid)
    lo = np.maximum(lo // micro, 0)
    hi = np.minimum(hi // micro, dims - 1)
    return lo, hi, (lo <= hi).all(axis=1)


def private_image_bytes(grid, micro, chunk_cells):
    """LDS bytes of bucketCountPrivateKernel's image for a top level of one chunk of chunk_cells cells a side: 16 bits a
    microblock, a word per node of the coarser levels (bucket.hip, Bucketer::recurse)."""
    ext = np.asarray(grid["extents"], np.int64).reshape(3, 2)
    dims = (ext[:, 1] - ext[:, 0] + micro - 1) // micro
    levels = 1
    while (micro << (levels - 1)) < chunk_cells:
        levels += 1
    words = (int(dims.prod()) + 1) // 2
    for l in range(1, levels):
        words += int(((dims + (1 << l) - 1) >> l).prod())
    return 4 * words


FAR_FIRST = (2 ** 29 + 192, -2 ** 29 - 640, 2 ** 30)
FAR_CELLS = (2560, 2560, 5120)
FAR_STEP = (64, 64, 128)
FAR_BELOW = 300


def far(params, seed=11):
    """20 000 splats on a grid whose lower ends all lie at or beyond 2^29 cells: rangeOf's 64-bit branch for every splat.
    Positions are integer cells first + k * (64, 64, 128), k in 0 .. 39, which a float32 holds exactly (its ulp is 64 below
    2^30 and 128 from 2^30 on)."""
    rng = np.random.default_rng(seed)
    n = 20_000
    first = np.asarray(FAR_FIRST, np.int64)
    k = rng.integers(0, 40, (n + FAR_BELOW, 3))
    radius = rng.choice([10.0, 100.0, 200.0], n + FAR_BELOW)
    # ... and FAR_BELOW more one step below the grid on x or y, radius 10: their upper cell is first - 64 (float32 has no
    # first - 54), so they belong to no leaf, by the floor division of a NEGATIVE cell wherever a microblock is wider than 64
    k[n:][np.arange(FAR_BELOW), np.arange(FAR_BELOW) % 2] = -1
    radius[n:] = 10.0
    order = rng.permutation(n + FAR_BELOW)
    cells = (first + k * np.asarray(FAR_STEP, np.int64))[order]
    s = _splats(cells, radius[order])
    assert np.array_equal(s["position"].astype(np.int64), cells)
    ext = tuple(int(v) for a in range(3) for v in (first[a], first[a] + FAR_CELLS[a]))
    return s, dict(reference=(0.0, 0.0, 0.0), spacing=1.0, extents=ext), _params(*params)


GIANTS = (((0, 0, 0), 5e9), ((10, 10, 10), 1e12), ((3e9, 5, 5), 1), ((-3e9, 5, 5), 2), ((-3e9, 0, 0), 3.5e9),
          ((5, 2e12, 5), 1), ((5, 5, -1e10), 1.0001e10), ((1e9, 1e9, 1e9), 1))


def giants(params, seed=12):
    """An ordinary cloud, cut off by its grid, with eight splats of 10^9 .. 10^12 cells among it: some cover the whole
    grid, some lie that far away -- the 64-bit branch taken per SPLAT on a grid that is itself narrow.  Every |cell| stays
    below 10^13."""
    rng = np.random.default_rng(seed)
    n = 15_000
    pos = np.concatenate([rng.uniform(-40.0, 60.0, (n, 3)), np.asarray([g[0] for g in GIANTS], np.float64)])
    rad = np.concatenate([rng.uniform(0.05, 1.5, n), np.asarray([g[1] for g in GIANTS], np.float64)])
    s = _splats(pos, rad)[rng.permutation(n + len(GIANTS))]
    grid = dict(reference=(1.5, 0.0, -2.25), spacing=0.5, extents=(-90, 130, -85, 125, -80, 120))
    return s, grid, _params(*params)


SPANS_CELLS = 72


def spans(micro, seed=13):
    """Small splats, 40 balls of 34 .. 60 cells, 40 balls of the whole grid and 40 splats that are as long on ONE axis and
    at most two cells on the others (a ball has one radius: they hang outside two faces of the grid, which cuts them down
    to its first cells), shuffled.  72 cells a side: 36 microblocks of 2 cells, so that a range can exceed 31 microblocks
    -- packNote's "does not fit" marker -- at micro 2 as well as 1, while 36^3 16-bit counters still fit the private
    kernel's LDS image."""
    rng = np.random.default_rng(seed)
    g = float(SPANS_CELLS)
    pos = [rng.uniform(0.0, g, (3000, 3)), rng.uniform(10.0, 54.0, (40, 3)), rng.uniform(g / 2 - 1, g / 2 + 1, (40, 3))]
    rad = [rng.uniform(0.05, 0.6, 3000), rng.uniform(17.0, 30.0, 40), rng.uniform(33.0, 36.0, 40)]
    r = rng.uniform(33.0, 36.0, 40)
    p = -r[:, None] + rng.uniform(0.2, 1.8, (40, 3))            # upper corner in cell 0 or 1, lower corner far outside
    axis = np.arange(40) % 3
    p[np.arange(40), axis] = rng.uniform(g / 2 - 1, g / 2 + 1, 40)
    s = _splats(np.concatenate(pos + [p]), np.concatenate(rad + [r]))
    s = s[rng.permutation(len(s))]
    grid = dict(reference=(0.0, 0.0, 0.0), spacing=1.0, extents=(0, SPANS_CELLS) * 3)
    return s, grid, _params(200, 16, 0, micro, 1 << 20)


CLUSTER_BLOCK = (1, 2, 1)       # the microblock (x, y, z) of 63 cells that holds the cluster


def cluster(seed=14):
    """150 000 splats inside ONE microblock of 63 cells and 5 000 ordinary ones.  In id order: PRIV_SPAN cluster splats
    -- the first workgroup of bucketCountPrivateKernel adds every element of its span to one 16-bit counter -- then the
    5 000, then the rest of the cluster."""
    rng = np.random.default_rng(seed)
    corner = 63.0 * np.asarray(CLUSTER_BLOCK, np.float64)
    inside = corner + rng.uniform(0.5, 62.5, (150_000, 3))
    wide = rng.uniform(1.0, 251.0, (5000, 3))
    pos = np.concatenate([inside[:PRIV_SPAN], wide, inside[PRIV_SPAN:]])
    rad = np.concatenate([np.full(PRIV_SPAN, 0.3), rng.uniform(0.3, 2.5, 5000), np.full(150_000 - PRIV_SPAN, 0.3)])
    grid = dict(reference=(0.0, 0.0, 0.0), spacing=1.0, extents=(0, 252) * 3)
    return _splats(pos, rad), grid, _params(5000, 255, 0, 63, 1 << 30)


BEYOND = (((0, 0, 0), 1e30), ((1e30, 0, 0), 1), ((-3e38,) * 3, 3e38), ((3e38,) * 3, 3e38))      # A, B, C, D
BEYOND_FIRST_ID = 5000          # A, B, C, D are splats 5000 .. 5003


def beyond(seed=15):
    """An ordinary cloud and four splats whose cells no int64 holds, all fields finite: A covers everything, B lies 10^30
    away, C's lower corner is -inf (upper corner: world 0) and D's upper corner +inf (lower corner: world 0)."""
    rng = np.random.default_rng(seed)
    ref = (-40.25, -50.5, -30.75)
    pos = np.concatenate([np.asarray(ref) + rng.uniform(0.0, 100.0, (BEYOND_FIRST_ID, 3)), np.asarray([b[0] for b in BEYOND], np.float64)])
    rad = np.concatenate([rng.uniform(0.1, 1.5, BEYOND_FIRST_ID), np.asarray([b[1] for b in BEYOND], np.float64)])
    s = _splats(pos, rad)
    assert np.isfinite(s["position"]).all() and np.isfinite(s["radius"]).all()
    return s, dict(reference=ref, spacing=1.0, extents=(0, 100) * 3), _params(500, 25, 0, 5, 1 << 20)


FAR_PARAMS = (300, 256, 0, 64, 1 << 20)
# the same leaves eight to a leaf: bucket_checks.validate_partition compares every pair of leaves
FAR_COARSE_PARAMS = (3000, 512, 0, 64, 1 << 20)

CASES = {
    "far": far(FAR_PARAMS),
    "far_chunks": far((300, 256, 1024, 0, 512)),
    "far_coarse": far(FAR_COARSE_PARAMS),
    "giants": giants((400, 48, 0, 16, 1 << 20)),
    "giants_chunks": giants((400, 48, 100, 0, 200)),
    "spans_micro1": spans(1),
    "spans_micro2": spans(2),
    "cluster": cluster(),
    "beyond": beyond(),
}
for _case in CASES.values():
    _case[0].setflags(write=False)
