"""Marching on the GPU at the extents the API accepts: rows of 32 to 8189 corners, 2049 rows a layer, 1031 slices a bucket, and
lock-step batches whose lanes differ in width, density and route.

Every marching kernel changes what it does with the row length (W corners, cw = W - 1 cells, nw = ceil((2 W - 1) / 64) lattice
words): latticeMaskWordKernel shares a wave among 64 / nw rows; latticeMaskKernel takes over at nw > 64, where the cells route
for triangles is forced too; latticeTrianglesRowKernel stages 9 nw words in LDS sized by the widest lane of the launch and
pipelines 64-cell chunks; cellCodeKernel works in rounds of 192 cells.  The cases (tests/marching_extent_cases.py, whose
conditions test_marching_extents_oracle.py asserts on the CPU) put every one of these on both sides of its thresholds.

Every run is held to the oracle's run of the same bucket: batches bit for bit (NaN positions compared first, as
test_gpu_fp64.py does) and the counters.  The device's own output on 2049-long grids is held to float64 as well.

64-bit weld keys (wideKeys, a key layout of more than 32 bits) are in test_gpu_marching_keys.py.  The layout is bit fields
plus a flag bit, bitsFor(2 (W - 1)) + bitsFor(2 (H - 1)) + bitsFor(2 (D - 1)) + 1 > 32, not the product (2 W)(2 H)(2 D): a
side of 2^(b - 2) + 1 corners takes b bits, so the route begins at 2^26 corners, 257 x 257 x 1025 for one; the case there is
257 x 257 x 1033 (internal vertices with the top bit of the z field), at a mesh-memory floor of 58 MB."""
import numpy as np
import pytest

import fp64_reference as fr
import marching_extent_cases as mx
from gpu_common import assert_batches_equal, ctx  # noqa: F401
from test_gpu_fp64 import _canon_nan
from test_marching_extents_oracle import check_wide_mesh

pytestmark = pytest.mark.gpu

MEMORIES = ("ample", "tight")


def make(ctx, case, memory):
    import mlsgpu_amd as m
    return m.Marching(ctx, case.dims[0], case.dims[1], case.dims[2], case.swathe, case.memory(memory), mx.ALIGNMENT)


def generate(ctx, mc, case, key_offset=mx.KEY_OFFSET):
    import mlsgpu_amd as m
    return mc.generate(m.binding.HostGenerator(ctx, case.fn, mx.ALIGNMENT), case.size, key_offset)


def assert_same(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for g, e in zip(got, exp):
        assert g["vertices"].shape == e["vertices"].shape, what
        np.testing.assert_array_equal(np.isnan(g["vertices"]), np.isnan(e["vertices"]), err_msg=str(what))
    assert_batches_equal(_canon_nan(got), _canon_nan(exp))


def assert_counters(mc, st, what, before=None):
    cnt = mc.counters()
    for k in mx.COUNTERS:
        assert cnt[k] - (before[k] if before else 0) == st[k], (what, k)
    return cnt


def check_case(ctx, case, memory, repeat=False, key_offset=mx.KEY_OFFSET):
    """One object, one generate (two with `repeat`: no stale device state) against the oracle's run of the case."""
    exp, st = mx.oracle_run(case, memory, key_offset)
    mc = make(ctx, case, memory)
    got = generate(ctx, mc, case, key_offset)
    assert_same(got, exp, (case, memory))
    cnt = assert_counters(mc, st, (case, memory))
    if repeat:
        assert_same(generate(ctx, mc, case, key_offset), exp, (case, memory, "again"))
        assert_counters(mc, st, (case, memory, "again"), cnt)
    return got


@pytest.mark.parametrize("width", sorted(mx.WIDTHS))
@pytest.mark.parametrize("field", ["noise", "tube"])
def test_every_width(ctx, field, width, monkeypatch):
    """Both fields at every width of WIDTHS, the route left to the rule (noise by rows, the tube by cells, either by cells
    from nw = 65), ample memory, key offset (7, 0, 3)."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    got = check_case(ctx, mx.width_case(field, width), "ample")
    assert len(got) == 1 and len(got[0]["triangles"]) > 100


@pytest.mark.parametrize("memory", MEMORIES)
@pytest.mark.parametrize("width", mx.REGIME_WIDTHS)
@pytest.mark.parametrize("field", ["noise", "tube"])
def test_regimes_routes_and_welds(ctx, field, width, memory, monkeypatch):
    """One width of every regime (nw 7, 15, 33, 64, 65) with the triangle route left to the rule, forced by rows and forced
    by cells, with the lattice and the sort weld, and twice on the same object.  At W = 2049 the cells route is forced, so all
    three settings must give the one result."""
    for weld in ("lattice", "sort"):
        case = mx.width_case(field, width, sort_buffers=weld == "sort")
        exp, st = mx.oracle_run(case, memory)
        mc = make(ctx, case, memory)
        if weld == "sort":
            monkeypatch.setenv("MLSGPU_HIP_WELD", "sort")
        else:
            monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
        cnt = None
        for route in (None, "0", "1"):
            if route is None:
                monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
            else:
                monkeypatch.setenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", route)
            for again in (False, True):
                what = (case, memory, weld, route, again)
                assert_same(generate(ctx, mc, case), exp, what)
                cnt = assert_counters(mc, st, what, cnt)
        del mc
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)


@pytest.mark.parametrize("width", (32, 33, 96, 130))
@pytest.mark.parametrize("field", ["noise", "tube"])
def test_mask_kernels_agree(ctx, field, width, monkeypatch):
    """latticeMaskWordKernel (the rule's choice up to nw 64) and latticeMaskKernel (MLSGPU_HIP_LATTICE_MASK_ROWS=1) on the
    same object, lattice weld, ample memory: both runs equal the oracle's, so the two kernels write the same lattice.  nw 1,
    2, 3 and 5 are the smallest rows at which they differ in structure: a wave of the word kernel shared by 64, 32, 21 and
    12 rows of corners, a last word that is nearly empty, the top column in word 0 and in the last word."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    case = mx.width_case(field, width)
    assert mx.lattice_words(width) == {32: 1, 33: 2, 96: 3, 130: 5}[width]
    exp, st = mx.oracle_run(case, "ample")
    mc = make(ctx, case, "ample")
    cnt = None
    for by_rows in (None, "1"):
        if by_rows is None:
            monkeypatch.delenv("MLSGPU_HIP_LATTICE_MASK_ROWS", raising=False)
        else:
            monkeypatch.setenv("MLSGPU_HIP_LATTICE_MASK_ROWS", by_rows)
        what = (case, "mask by rows", by_rows)
        assert_same(generate(ctx, mc, case), exp, what)
        cnt = assert_counters(mc, st, what, cnt)
    monkeypatch.delenv("MLSGPU_HIP_LATTICE_MASK_ROWS", raising=False)


@pytest.mark.parametrize("memory", MEMORIES)
@pytest.mark.parametrize("case", mx.EXTENT_CASES, ids=repr)
def test_tall_deep_and_wide_swathes(ctx, case, memory, monkeypatch):
    """2061 and 4097 lattice rows a layer; 1031 slices as one swathe (lattice weld) and as seventeen (sort weld, copy_slice
    between every pair); 2049 corners a row over three swathes."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    got = check_case(ctx, case, memory, repeat=True)
    assert sum(len(b["triangles"]) for b in got) > 100


@pytest.mark.parametrize("size", [(2049, 5, 4), (5, 2049, 4)], ids=lambda s: "%dx%dx%d" % tuple(s))
@pytest.mark.parametrize("field", ["noise", "tube"])
def test_device_output_vs_fp64(ctx, field, size, monkeypatch):
    """The device's own batches on grids 2049 corners long against marching_fp64 with the tolerance of every vertex's
    binade: nothing missing or extra, triangle count, orientation, the float32 formula pinned."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    case = mx.thin_case(field, size)
    got = check_case(ctx, case, "ample", key_offset=(0, 0, 0))
    ref = fr.marching_fp64(mx.field_array(case.fn, case.size))
    c = check_wide_mesh(got, ref, case.name)
    assert c["vertices"] > 10 * max(size)


def run_batch(ctx, cases, memory):
    import mlsgpu_amd as m
    marchings = [make(ctx, c, memory) for c in cases]
    gens = [m.binding.HostGenerator(ctx, c.fn, mx.ALIGNMENT) for c in cases]
    offsets = [(3 * k, 100 + k, 7 * k) for k in range(len(cases))]
    got = m.Marching.generate_batch(marchings, gens, [c.size for c in cases], offsets)
    return marchings, offsets, got


@pytest.mark.parametrize("memory", MEMORIES)
@pytest.mark.parametrize("name", sorted(mx.BATCHES))
def test_mixed_batches(ctx, name, memory, monkeypatch):
    """Lanes of different maximum sizes in one generate_batch: (a) rows-route lanes of nw 64 and 4 in one
    latticeTrianglesRowKernel launch (LDS sized by the wider, in either order), a cells-route lane and a lane without
    surface; (b) the same plus a lane of nw 65, which puts every lane on the wave-per-row mask kernel and itself on the cells
    route.  Every lane equals the oracle's run of that bucket alone, counters included."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    cases = mx.BATCHES[name]
    marchings, offsets, got = run_batch(ctx, cases, memory)
    assert len(got) == len(cases)
    for k, case in enumerate(cases):
        exp, st = mx.oracle_run(case, memory, offsets[k])
        assert_same(got[k], exp, (name, case, memory))
        assert_counters(marchings[k], st, (name, case, memory))
        assert (len(exp) == 0) == (case.field == "positive")


@pytest.mark.parametrize("memory", MEMORIES)
def test_batch_of_one_equals_generate(ctx, memory, monkeypatch):
    """Every lane of batch (b) alone: generate_batch of the one object gives what generate gives."""
    import mlsgpu_amd as m
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    for case in mx.BATCH_B:
        exp, st = mx.oracle_run(case, memory)
        mc = make(ctx, case, memory)
        gen = m.binding.HostGenerator(ctx, case.fn, mx.ALIGNMENT)
        one = m.Marching.generate_batch([mc], [gen], [case.size], [mx.KEY_OFFSET])
        assert len(one) == 1
        assert_same(one[0], exp, (case, memory, "batch of one"))
        cnt = assert_counters(mc, st, (case, memory, "batch of one"))
        assert_same(generate(ctx, mc, case), one[0], (case, memory, "generate"))
        assert_counters(mc, st, (case, memory, "generate"), cnt)
        del mc
