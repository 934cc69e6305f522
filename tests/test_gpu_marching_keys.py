"""The sort weld of marching.hip at compact keys of 31 to 34 bits: the 32-bit route with its flag in bit 31 and the 64-bit route
(generateElementsKernel<uint64_t>, radixSort<uint64_t>, UniqueIn<uint64_t>, CompactVerticesOut<uint64_t>), which beginGenerate
takes above 32 bits.

The grids (tests/marching_key_cases.py, whose conditions test_marching_keys_oracle.py asserts on the CPU) are the cheapest with
their bit counts: about 2^26 corners, 2^27 at 34 bits, noise in two columns and a patch, mesh memory at the constructor's
floor.  Every run is held to the oracle's run of the same bucket, batches bit for bit and the seven counters; nothing is
compared with another device run only."""
import pytest

import marching_extent_cases as mx
import marching_key_cases as mk
from gpu_common import ctx  # noqa: F401
from test_gpu_marching_extents import assert_counters, assert_same, check_case, generate, make

pytestmark = pytest.mark.gpu

SORT_STAT = "kernel.marching.sortVertices.time"


def report(case):
    """The time of the oracle's run of the case, made here unless an earlier test has (check_case then finds it cached)"""
    print("%s: oracle %.2f s" % (case.name, mk.oracle_seconds(case)))


@pytest.mark.parametrize("name", mk.NAMES)
def test_sort_weld_across_swathes(ctx, name, monkeypatch):
    """Several swathes a bucket (5, 3 or 17), copy_slice between them, ship-outs in the middle of the bucket: batches and
    counters equal the oracle's, and again on the same object (no stale key scratch of either width)."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    case = mk.case(name, "swathes")
    report(case)
    got = check_case(ctx, case, mk.MEMORY, repeat=True)
    assert sum(len(b["triangles"]) for b in got) > 100


@pytest.mark.parametrize("name", mk.ONE)
def test_lattice_weld_same_grids(ctx, name, monkeypatch):
    """The same grids in one swathe: the lattice weld, into which no key layout enters, on slices of 512 x 512 cells and
    buckets of 1033 slices."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    case = mk.case(name, "one")
    report(case)
    got = check_case(ctx, case, mk.MEMORY)
    assert sum(len(b["triangles"]) for b in got) > 100


@pytest.mark.parametrize("name", mk.FORCED)
def test_forced_sort_one_swathe(ctx, name, monkeypatch):
    """MLSGPU_HIP_WELD=sort on a bucket of one swathe whose mesh the floor holds: one ship-out, hence ONE sort of all its
    unwelded vertices.  The route is told from the context's statistics: with timing on, every launch of the radix sort is a
    sample of kernel.marching.sortVertices.time -- three a pass, four passes -- and the lattice weld launches none."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_SORT_DIGIT_BITS", raising=False)       # the tuning aid changes the pass split counted below
    monkeypatch.setenv("MLSGPU_HIP_WELD", "sort")
    case = mk.case(name, "forced")
    report(case)
    exp, st = mk.oracle_run(case)
    assert st["shipouts"] == 1
    mc = make(ctx, case, mk.MEMORY)
    ctx.reset_stats()
    ctx.set_timing(True)
    try:
        got = generate(ctx, mc, case)
    finally:
        ctx.set_timing(False)
    launches = ctx.stats().get(SORT_STAT, (0.0, 0))[1]
    ctx.reset_stats()
    assert_same(got, exp, (case, "forced"))
    cnt = assert_counters(mc, st, (case, "forced"))
    assert cnt["shipouts"] == 1 and cnt["overflows"] == 0
    assert launches == mk.sort_launches(case.size), launches
    # ... and without the setting the same object takes the lattice weld: no sort launch, the same batches
    monkeypatch.delenv("MLSGPU_HIP_WELD")
    ctx.set_timing(True)
    try:
        again = generate(ctx, mc, case)
    finally:
        ctx.set_timing(False)
    launches = ctx.stats().get(SORT_STAT, (0.0, 0))[1]
    ctx.reset_stats()
    assert launches == 0
    assert_same(again, exp, (case, "lattice"))
    assert_counters(mc, st, (case, "lattice"), cnt)


def test_wide_lane_in_a_batch(ctx, monkeypatch):
    """generate_batch over a lane of 64-bit keys, a narrow one and a lane of 32-bit keys with the flag in bit 31 (lanes of
    several swathes are taken bucket by bucket): every lane equals the oracle's run of that bucket alone, the narrow lane
    between two key types included."""
    import mlsgpu_amd as m
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    lanes = [(mk.case("k33_deep", "swathes"), mk.MEMORY, mx.KEY_OFFSET),
             (mx.BATCH_A[1], "ample", (3, 101, 7)),
             (mk.case("k32_a", "swathes"), mk.MEMORY, mx.KEY_OFFSET)]
    marchings = [make(ctx, case, memory) for case, memory, _ in lanes]
    gens = [m.binding.HostGenerator(ctx, case.fn, mx.ALIGNMENT) for case, _, _ in lanes]
    got = m.Marching.generate_batch(marchings, gens, [case.size for case, _, _ in lanes], [off for _, _, off in lanes])
    assert len(got) == len(lanes)
    for k, (case, memory, off) in enumerate(lanes):
        exp, st = mx.oracle_run(case, memory, off)
        assert len(exp) >= 1
        assert_same(got[k], exp, (case, "lane", k))
        assert_counters(marchings[k], st, (case, "lane", k))
