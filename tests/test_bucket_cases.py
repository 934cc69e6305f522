"""The bucketer's constructed clouds (bucket_cases.py) do what they are for -- each reaches the branch of
mlsgpu_amd/csrc/bucket.hip it was built to reach -- and the oracle's leaves of every one of them are a partition
(bucket_checks.validate_partition)."""
import functools

import numpy as np
import pytest

import bucket_cases as bc
import bucket_checks
import oracle_binding as ob
from bucket_checks import cell_box, random_case, validate_partition

# validate_partition compares every pair of leaves: `far` and `far_chunks` (2 000 leaves) are validated as `far_coarse`
VALIDATED = [name for name in bc.CASES if name not in ("far", "far_chunks")]


@functools.lru_cache(maxsize=None)
def oracle_leaves(name):
    splats, grid, p = bc.CASES[name]
    return ob.bucket_partition(splats, grid["reference"], grid["spacing"], grid["extents"], p["max_splats"], p["max_cells"],
                               p["chunk_cells"], p["micro_cells"], p["max_split"])        # raises DensityError if one cell is too dense


def members(name):
    """[leaves, splats] bool: is the splat listed in the leaf?"""
    leaves = oracle_leaves(name)
    m = np.zeros((len(leaves), len(bc.CASES[name][0])), bool)
    for i, leaf in enumerate(leaves):
        m[i, leaf["ids"].astype(np.int64)] = True
    return m


def grid_cells(grid):
    ext = np.asarray(grid["extents"], np.int64).reshape(3, 2)
    return ext[:, 1] - ext[:, 0]


@pytest.mark.parametrize("name", list(bc.CASES))
def test_oracle_makes_leaves_without_density_error(name):
    leaves = oracle_leaves(name)
    assert len(leaves) > 1
    assert sum(len(leaf["ids"]) for leaf in leaves) >= np.count_nonzero(bc.micro_range(*bc.CASES[name][:2], 1)[2])


@pytest.mark.parametrize("name", VALIDATED)
def test_oracle_leaves_are_a_partition(name, monkeypatch):
    splats, grid, p = bc.CASES[name]
    if name == "beyond":        # boxes that no int64 holds: the checker's boxes take the clamp the bucketers take
        monkeypatch.setattr(bucket_checks, "cell_box", bc.cell_box_clamped)
    leaves = oracle_leaves(name)
    assert len(leaves) <= 600
    validate_partition(splats, grid, leaves, p["max_splats"], p["max_cells"], 0, strict=False)


def test_clamped_box_is_the_box_wherever_the_box_is_defined():
    for seed in range(30):
        splats, grid, _ = random_case(seed)
        for a, b in zip(cell_box(splats, grid), bc.cell_box_clamped(splats, grid)):
            np.testing.assert_array_equal(a, b)
    for name in ("far", "giants", "spans_micro1", "cluster"):
        splats, grid, _ = bc.CASES[name]
        for a, b in zip(cell_box(splats, grid), bc.cell_box_clamped(splats, grid)):
            np.testing.assert_array_equal(a, b)
        assert np.abs(np.stack(cell_box(splats, grid))).max() < 1e13          # float64 and int64 alike hold these exactly


def test_far_grid_takes_the_wide_branch():
    splats, grid, p = bc.CASES["far"]
    first = np.asarray(grid["extents"], np.int64).reshape(3, 2)[:, 0]
    assert (np.abs(first) >= bc.NARROW_FIRST).all()
    assert tuple(first) == bc.FAR_FIRST and tuple(grid_cells(grid)) == bc.FAR_CELLS
    # positions are whole cells, exactly: first + k * step
    k = (splats["position"].astype(np.float64) - first) / np.asarray(bc.FAR_STEP, np.float64)
    assert np.array_equal(k, np.round(k)) and k.min() == -1 and k.max() == 39
    below = (k < 0).any(axis=1)
    assert (~below).sum() == 20_000 and below.sum() == bc.FAR_BELOW
    assert np.array_equal(splats["position"], splats["position"].astype(np.int64).astype(np.float32))
    assert set(np.unique(splats["radius"]).tolist()) == {10.0, 100.0, 200.0}
    lo, hi = cell_box(splats, grid)
    # the ones below the grid end one float32 step below its first cell, on x and on y: the floor division of a negative
    # cell by a microblock of more than 64 cells (far_chunks) keeps them out
    assert (hi[below].min(axis=1) == -64).all() and {0, 1} == set(np.argmin(hi[below], axis=1).tolist())
    assert (hi[~below] >= 0).all() and (lo[~below] < grid_cells(grid)).all()
    for name in ("far", "far_chunks", "far_coarse"):
        assert not members(name)[:, below].any()
    assert (lo + first)[:, 2].min() >= bc.NARROW_CELL                   # on z the cells themselves are beyond 1e9 too
    # every top-level region is a leaf, and there are more of them than one sort digit numbers
    leaves = oracle_leaves("far")
    assert all(leaf["depth"] == 1 for leaf in leaves)
    assert len(leaves) == 2000 > 1 << bc.SORT_MAX_DIGIT_BITS
    for other in ("far_chunks", "far_coarse"):
        assert bc.CASES[other][0].tobytes() == splats.tobytes() and bc.CASES[other][1] == grid
    chunked = oracle_leaves("far_chunks")
    assert {leaf["depth"] for leaf in chunked} == {2} and len({leaf["chunk"] for leaf in chunked}) > 8
    assert 100 < len(oracle_leaves("far_coarse")) <= 600


@pytest.mark.parametrize("name", ["giants", "giants_chunks"])
def test_giants_cover_or_miss_the_grid(name):
    splats, grid, p = bc.CASES[name]
    first = np.asarray(grid["extents"], np.int64).reshape(3, 2)[:, 0]
    for a in first:
        assert abs(int(a)) < bc.NARROW_FIRST            # the grid itself is narrow
    cells = grid_cells(grid)
    lo, hi = cell_box(splats, grid)
    assert max(np.abs(lo).max(), np.abs(hi).max()) < 1e13
    covers = ((lo <= 0) & (hi >= cells - 1)).all(axis=1)
    gap = np.maximum(lo - (cells - 1), -hi).max(axis=1)                 # cells between the box and the grid
    misses = gap > 1_000_000_000
    meets = ((hi >= 0) & (lo <= cells - 1)).all(axis=1)
    big = np.maximum(np.abs(lo + first), np.abs(hi + first)).max(axis=1) >= bc.NARROW_CELL
    assert covers.sum() >= 4 and misses.sum() >= 3 and (big & meets).sum() >= 1
    assert (big == (covers | misses)).all() and big.sum() == len(bc.GIANTS)
    assert (~meets & ~big).sum() > 100 and (meets & ~covers).sum() > 10_000     # the grid cuts the ordinary cloud off
    m = members(name)
    assert len(m) == 343
    assert m[:, covers].all() and not m[:, misses].any()
    depths = {leaf["depth"] for leaf in oracle_leaves(name)}
    assert depths == ({1} if name == "giants" else {1, 2})


@pytest.mark.parametrize("micro", [1, 2])
def test_spans_exceed_what_a_kept_range_holds(micro):
    splats, grid, p = bc.CASES["spans_micro%d" % micro]
    assert p["micro_cells"] == micro
    blocks = (grid_cells(grid) + micro - 1) // micro
    assert (blocks > bc.NOTE_MAX_SPAN + 1).all()
    lo, hi, meets = bc.micro_range(splats, grid, micro)
    assert meets.all()
    span = hi - lo
    wide = span > bc.NOTE_MAX_SPAN
    assert (wide.all(axis=1)).sum() >= 40
    one_axis = (wide.sum(axis=1) == 1) & ((span <= 1).sum(axis=1) == 2)
    assert one_axis.sum() >= 40
    assert set(np.argmax(wide[one_axis], axis=1).tolist()) == {0, 1, 2}         # along each axis
    assert ((span > 1).any(axis=1) & ~wide.any(axis=1)).sum() >= (40 if micro == 1 else 1)      # the general loops, range kept
    assert (span <= 1).all(axis=1).sum() >= 2500                                # and the two-per-axis fast path
    assert (lo <= 0xFFFF).all()
    # the private counters take the level at 2 cells a microblock (36^3 16-bit counters); at 1 the plain kernel does
    chunk = -(-int(grid_cells(grid).max()) // p["max_cells"]) * p["max_cells"]      # one chunk, rounded up to whole leaves
    image = bc.private_image_bytes(grid, micro, chunk)
    assert (image <= bc.PRIV_LDS_BYTES) == (micro == 2)
    assert len(oracle_leaves("spans_micro%d" % micro)) == 125


def test_cluster_fills_one_counter_of_the_first_span():
    splats, grid, p = bc.CASES["cluster"]
    micro = p["micro_cells"]
    assert micro == 63 and tuple(grid_cells(grid)) == (252, 252, 252)
    assert bc.PRIV_SPAN == 63 * 1024 < 1 << 16
    lo, hi, meets = bc.micro_range(splats, grid, micro)
    assert meets.all()
    block = np.asarray(bc.CLUSTER_BLOCK)
    assert (lo[:bc.PRIV_SPAN] == block).all() and (hi[:bc.PRIV_SPAN] == block).all()       # the counter reaches PRIV_SPAN
    x, y, z = bc.CLUSTER_BLOCK
    index = (z * 4 + y) * 4 + x
    assert index % 2 == 1                                               # the high half of its LDS word
    neighbour = np.asarray((x - 1, y, z))                               # the low half of the same word
    assert ((z * 4 + y) * 4 + x - 1) // 2 == index // 2
    hits = ((lo <= neighbour) & (neighbour <= hi)).all(axis=1)
    assert hits[:bc.PRIV_SPAN + 5000].any() and not hits[:bc.PRIV_SPAN].any()
    assert hits[bc.PRIV_SPAN:bc.PRIV_SPAN + 5000].sum() > 10
    assert bc.private_image_bytes(grid, micro, 252) <= bc.PRIV_LDS_BYTES
    leaves = oracle_leaves("cluster")
    assert max(leaf["depth"] for leaf in leaves) == 2 and len(leaves) > 50


def test_beyond_boxes_reach_past_every_integer():
    splats, grid, p = bc.CASES["beyond"]
    ids = np.arange(bc.BEYOND_FIRST_ID, bc.BEYOND_FIRST_ID + 4)
    a, b, c, d = ids
    assert np.isfinite(splats["position"]).all() and np.isfinite(splats["radius"]).all()
    with np.errstate(over="ignore"):
        low = splats["position"] - splats["radius"][:, None]
        high = splats["position"] + splats["radius"][:, None]
    assert (low[c] == -np.inf).all() and (high[c] == 0).all() and (high[d] == np.inf).all() and (low[d] == 0).all()
    assert np.abs(low[a]).min() >= 2.0 ** 63 and np.abs(high[a]).min() >= 2.0 ** 63 and low[b, 0] >= 2.0 ** 63
    lo, hi = bc.cell_box_clamped(splats, grid)
    assert np.abs(np.stack([lo[:a], hi[:a]])).max() < 200                # the ordinary ones are ordinary
    assert p["max_splats"] >= 2 * (4 + max(len(leaf["ids"]) for leaf in oracle_leaves("beyond")))
    # world 0 lies in this cell of the grid (the grid's first cell is 0)
    zero = np.floor((np.float32(0) - np.asarray(grid["reference"], np.float32)) * (np.float32(1) / np.float32(grid["spacing"])))
    zero = zero.astype(np.int64)
    assert (zero > 0).all() and (zero < grid_cells(grid) - 1).all()
    m = members("beyond")
    ext = np.asarray([leaf["extents"] for leaf in oracle_leaves("beyond")], np.int64).reshape(-1, 3, 2)
    assert m[:, a].all() and not m[:, b].any()
    want_c = (ext[:, :, 0] <= zero).all(axis=1)                         # the leaf has a cell <= zero on every axis
    want_d = (ext[:, :, 1] - 1 >= zero).all(axis=1)                     # ... a cell >= zero
    assert np.array_equal(m[:, c], want_c) and np.array_equal(m[:, d], want_d)
    assert 0 < want_c.sum() < len(m) and 0 < want_d.sum() < len(m) and (want_c & want_d).sum() >= 1
    # the single-splat mapping, as the reference's splatToBuckets vectors pin it for ordinary splats
    for i, (wl, wh) in ((a, (-2 ** 62, 2 ** 62)), (c, (-2 ** 62, None)), (d, (None, 2 ** 62))):
        l, h = ob.splat_to_buckets(splats[i], grid["reference"], grid["spacing"], grid["extents"], 1)
        assert wl is None or (l == wl).all()
        assert wh is None or (h == wh).all()
        assert wl is not None or (l == zero).all()
        assert wh is not None or (h == zero).all()
