"""HIP bucketer on the constructed clouds of bucket_cases.py (far grids, giant splats, ranges of more than 31 microblocks,
a counting span in one microblock, boxes no integer holds): the oracle's leaves -- extents, chunk, depth, ids in order --
on every path a level can take; the loader's transform on the far grid; the bounding grid at the ends of int32.
tests/test_bucket_cases.py asserts, without a GPU, that each cloud reaches the branch it is here for."""
import numpy as np
import pytest

import bucket_cases as bc
import oracle_binding as ob
from bucket_checks import create_splats
from test_gpu_bucketer import both

pytestmark = pytest.mark.gpu

# cases with a level that bucketCountPrivateKernel takes once MLSGPU_HIP_BUCKET_PRIVATE_FROM lets it: at least two levels of
# counters that fit its LDS image (`far` itself has 40 x 40 x 80 microblocks: too many; its chunks have 2 x 2 x 2)
PRIVATE_CASES = ["cluster", "spans_micro2", "giants", "far_chunks"]


def run(name, ctx=None):
    splats, grid, p = bc.CASES[name]
    got, exp = both(splats, grid, p["max_splats"], p["max_cells"], p["chunk_cells"], p["micro_cells"], p["max_split"], ctx=ctx)
    assert got is not None and len(got) > 1
    return got


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_equals_oracle(name):
    run(name)


@pytest.mark.parametrize("private", ["0", "off"])
@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_with_kept_ranges_and_private_counters(name, private, monkeypatch):
    """Every element's range kept for the member-list passes (the spans cases: ranges that do not fit a note are marked
    and worked out again) and, with "0", per-workgroup 16-bit counters wherever they fit (cluster: one of them takes a whole
    span; spans_micro2: the loops over many nodes; giants, far_chunks: the corrections behind the 64-bit cell arithmetic)."""
    monkeypatch.setenv("MLSGPU_HIP_BUCKET_NOTES_FROM", "0")
    monkeypatch.setenv("MLSGPU_HIP_BUCKET_PRIVATE_FROM", private)
    run(name)


@pytest.mark.parametrize("name", PRIVATE_CASES)
def test_private_counters_are_engaged(name, monkeypatch):
    """The private path is three launches (count, slice sum, upsweep) where the plain one is one: the switch reaches the
    case, and the leaves do not depend on it."""
    import mlsgpu_amd as m
    monkeypatch.setenv("MLSGPU_HIP_BUCKET_NOTES_FROM", "0")
    launches, leaves = {}, {}
    for private in ("0", "off"):
        monkeypatch.setenv("MLSGPU_HIP_BUCKET_PRIVATE_FROM", private)
        ctx = m.Context(0)
        try:
            ctx.set_timing(True)
            ctx.reset_stats()
            leaves[private] = run(name, ctx=ctx)
            ctx.synchronize()
            launches[private] = ctx.stats().get("bucket.count.time", (0.0, 0))[1]
        finally:
            ctx.close()
    print("%s: %d count launches with private counters, %d without" % (name, launches["0"], launches["off"]))
    assert launches["0"] > launches["off"] > 0
    assert (launches["0"] - launches["off"]) % 2 == 0
    assert len(leaves["0"]) == len(leaves["off"])
    for x, y in zip(leaves["0"], leaves["off"]):
        assert x["extents"] == y["extents"] and x["chunk"] == y["chunk"] and x["depth"] == y["depth"]
        np.testing.assert_array_equal(x["ids"], y["ids"])


@pytest.mark.parametrize("forced", [False, True])
def test_one_context_case_after_case(forced, monkeypatch):
    """The scratch of a context regrows from case to case -- 373 248 microblocks of counters for 3 120 splats, then 64 for
    155 000, and back; lists, notes and slices likewise -- and every result stays the oracle's."""
    import mlsgpu_amd as m
    if forced:
        monkeypatch.setenv("MLSGPU_HIP_BUCKET_NOTES_FROM", "0")
        monkeypatch.setenv("MLSGPU_HIP_BUCKET_PRIVATE_FROM", "0")
    ctx = m.Context(0)
    try:
        for name in ("spans_micro1", "cluster", "spans_micro1", "far_chunks", "beyond", "giants_chunks", "spans_micro2", "far"):
            run(name, ctx=ctx)
    finally:
        ctx.close()


def test_load_on_the_far_grid():
    """mlsgpu_hip_bucket_load for the first, a middle and the last leaf of `far` against the transform written out in
    float32 numpy: (p - ref) * inv - float32(first), r * inv -- bit for bit."""
    import mlsgpu_amd as m
    from mlsgpu_amd import binding as b
    splats, grid, p = bc.CASES["far"]
    ref, spacing, extents = grid["reference"], grid["spacing"], grid["extents"]
    first = [extents[0], extents[2], extents[4]]
    assert all(int(np.float32(v)) == v for v in first)                  # the kernel subtracts float(first): nothing is lost
    exp = ob.bucket_partition(splats, ref, spacing, extents, p["max_splats"], p["max_cells"], p["chunk_cells"],
                              p["micro_cells"], p["max_split"])
    picked = (0, len(exp) // 2, len(exp) - 1)
    ctx = m.Context(0)
    dev = m.DeviceBuffer(ctx, array=splats)
    staged = m.DeviceBuffer(ctx, nbytes=p["max_splats"] * 32)
    loaded, seen = {}, [0]

    def on_bucket(leaf, d_ids):
        if seen[0] in picked:
            b.bucket_load(ctx, dev, d_ids, leaf["num_splats"], ref, spacing, extents, staged)
            loaded[seen[0]] = staged.download(m.SPLAT_DTYPE, leaf["num_splats"]).copy()
        seen[0] += 1
    try:
        got = b.bucket_cloud(ctx, dev, len(splats), ref, spacing, extents, p["max_splats"], p["max_cells"], p["chunk_cells"],
                             p["micro_cells"], p["max_split"], on_bucket=on_bucket)
    finally:
        dev.free()
        ctx.close()
    assert len(got) == len(exp) and sorted(loaded) == sorted(picked)
    inv = np.float32(1) / np.float32(spacing)
    for i in picked:
        assert got[i]["extents"] == exp[i]["extents"] and got[i]["num_splats"] == len(exp[i]["ids"]) > 0
        want = splats[exp[i]["ids"].astype(np.int64)].copy()
        want["position"] = (want["position"] - np.asarray(ref, np.float32)) * inv - np.asarray(first, np.float32)
        want["radius"] = want["radius"] * inv
        assert want["position"].dtype == np.float32
        np.testing.assert_array_equal(loaded[i].view(np.uint32), want.view(np.uint32))
        assert np.abs(want["position"]).max() < 6000                    # grid coordinates, not cells beyond 2^29


def expected_bounding(s, spacing, bucket):
    """FastBlobSet::makeBoundingGrid as tests/test_gpu_bucketer.py::test_bounding_grid states it"""
    spacing = np.float32(spacing)
    lo = np.floor((s["position"] - s["radius"][:, None]).min(axis=0) / spacing).astype(np.int64) // bucket * bucket
    hi = np.ceil((s["position"] + s["radius"][:, None]).max(axis=0) / spacing).astype(np.int64)
    return tuple(int(v) for v in (lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]))


def cloud_of(*rows):
    s = np.zeros(len(rows), ob.SPLAT_DTYPE)
    for i, (position, radius) in enumerate(rows):
        s["position"][i] = position
        s["radius"][i] = radius
    s["normal"] = (1.0, 0.0, 0.0)
    s["quality"] = 1.0
    assert np.isfinite(s["position"]).all() and np.isfinite(s["radius"]).all()
    return s


def test_bounding_grid_at_the_ends_of_int32():
    """Extents are int32: the last values that fit are returned, a cloud that needs more is refused with LengthError --
    also when only the rounding to the bucket size leaves int32, or when position + radius of a finite splat is infinite --
    and the context goes on working."""
    import mlsgpu_amd as m
    from mlsgpu_amd import binding as b
    small = create_splats()
    ctx = m.Context(0)
    held = []

    def grid_of(s, spacing, bucket):
        held.append(m.DeviceBuffer(ctx, array=s))
        return b.bounding_grid(ctx, held[-1], len(s), spacing, bucket)

    def refused(s, spacing, bucket):
        with pytest.raises(m.LengthError):
            grid_of(s, spacing, bucket)
        ref, sp, ext = grid_of(small, 0.5, 7)                           # ... and a small correct call succeeds
        assert ref == (0.0, 0.0, 0.0) and sp == 0.5 and ext == expected_bounding(small, 0.5, 7)
    try:
        top = 2147483520                                                # the largest float32 below 2^31
        assert np.float32(top) == top and np.nextafter(np.float32(top), np.float32(np.inf)) == 2.0 ** 31
        s = cloud_of(((top - 128, 0, 0), 128), ((0, 0, 0), 1))
        ref, sp, ext = grid_of(s, 1.0, 64)
        assert ext == expected_bounding(s, 1.0, 64) and ext[1] == top and ext[0] == -64

        refused(cloud_of(((3e9, 0, 0), 1)), 1.0, 1)

        s = cloud_of(((-2.0 ** 31 + 256, 0, 0), 256))
        assert s["position"][0, 0] - s["radius"][0] == -2.0 ** 31
        ref, sp, ext = grid_of(s, 1.0, 64)
        assert ext == expected_bounding(s, 1.0, 64) and ext[0] == -2147483648 and ext[1] == -2147483648 + 512
        assert expected_bounding(s, 1.0, 7)[0] < -2 ** 31               # the next multiple of 7 below is not an int32
        refused(s, 1.0, 7)

        s = cloud_of(((3e38, 0, 0), 3e38))
        with np.errstate(over="ignore"):
            assert s["position"][0, 0] + s["radius"][0] == np.inf
        refused(s, 1.0, 1)
        s = cloud_of(((-3e38, 5, 5), 3e38), ((1, 2, 3), 1))
        refused(s, 1.0, 64)                                             # a lower corner of -inf
    finally:
        for d in held:
            d.free()
        ctx.close()
