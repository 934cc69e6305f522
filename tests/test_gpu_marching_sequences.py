"""One marching object across a sequence of unlike buckets, as a worker's object lives: created at the maximum, then marched on
buckets of other widths, heights, depths, densities, welds and key widths, one after the other.

beginGenerate sets layout, wideKeys, direct, offsets, zTop and zBias per call; the field image (pitch and slice stride from the
maximum dims), the lattice words and rows, the cell codes, the 32/64-bit key scratch and the slice histogram keep what the
bucket before left.  A kernel that reads one element past the current width, row, slice or record count finds zeros on a fresh
object -- which is all the other marching tests give it -- and a plausible stale surface on a used one.

The expectation of every step is the oracle's run of that bucket on a FRESH object of the sequence object's dims, swathe and
mesh memory (marching_sequence_cases.oracle_step): batches bit for bit after the NaN canonicalisation of
test_gpu_marching_extents.assert_same, and the DELTAS of the seven counters.  No tolerance, and never a fresh device object per
step.  The conditions that keep this from passing vacuously (routes, welds, overflows, a surface left behind where the next step
does not reach, what the poisoning generators upload) are asserted on the CPU by test_marching_sequences_oracle.py."""
import time

import numpy as np
import pytest

import marching_extent_cases as mx
import marching_key_cases as mk
import marching_sequence_cases as ms
from gpu_common import assert_batches_equal, ctx  # noqa: F401
from test_gpu_marching_extents import assert_counters, assert_same

pytestmark = pytest.mark.gpu

SORT_STAT = "kernel.marching.sortVertices.time"


def make(ctx, obj, memory):
    import mlsgpu_amd as m
    return m.Marching(ctx, obj.dims[0], obj.dims[1], obj.dims[2], obj.swathe, obj.memory(memory), mx.ALIGNMENT)


def generator(ctx, obj, step, poison=None):
    """binding.HostGenerator (zeros in the padding columns, nothing in the padding rows) or a poisoning generator"""
    import mlsgpu_amd as m
    if poison is None:
        return m.binding.HostGenerator(ctx, step.fn, mx.ALIGNMENT)
    return ms.PoisonGenerator(ctx, obj, step.fn, poison)


def march(ctx, mc, obj, step, monkeypatch, poison=None):
    """One step on the object; MLSGPU_HIP_WELD=sort for this call alone where the step forces the sort weld"""
    gen = generator(ctx, obj, step, poison)
    if step.force_sort:
        monkeypatch.setenv("MLSGPU_HIP_WELD", "sort")
    try:
        got = mc.generate(gen, step.size, step.key_offset)
    finally:
        monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    if poison is not None:
        assert gen.error is None and gen.blocks == step.size[2]         # every slice's block was uploaded, once
    return got


def check_step(ctx, mc, obj, step, memory, monkeypatch, before, what, poison=None):
    """A step against the oracle's run of it on a fresh object: batches and counter deltas.  Returns (batches, counters)."""
    exp, st = ms.oracle_step(obj, step, memory)
    got = march(ctx, mc, obj, step, monkeypatch, poison)
    assert_same(got, exp, what)
    assert (len(got) == 0) == (not step.surface), what
    return got, assert_counters(mc, st, what, before)


def run_sequence(ctx, obj, steps, memory, monkeypatch, poison=None, weld_launches=False):
    """The steps in order on ONE object.  With weld_launches every step runs with timing on and its radix-sort launches are
    counted: some for a sort-weld step, none for a lattice one (MLSGPU_HIP_WELD must neither stick nor fail to take)."""
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    mc = make(ctx, obj, memory)
    cnt = mc.counters()
    assert not any(cnt.values())
    outs = []
    for i, step in enumerate(steps):
        what = (obj, memory, poison, i, step)
        if weld_launches:
            ctx.reset_stats()
            ctx.set_timing(True)
        try:
            got, cnt = check_step(ctx, mc, obj, step, memory, monkeypatch, cnt, what, poison)
        finally:
            if weld_launches:
                ctx.set_timing(False)
        if weld_launches:
            launches = ctx.stats().get(SORT_STAT, (0.0, 0))[1]
            ctx.reset_stats()
            assert (launches > 0) == (step.weld == "sort" and step.surface), (what, launches)
        outs.append(got)
    return mc, outs


def assert_bytes_equal(a, b, what):
    assert len(a) == len(b) >= 1, what
    for x, y in zip(a, b):
        assert x["num_internal"] == y["num_internal"], what
        for k in ("vertices", "triangles", "keys"):
            assert x[k].tobytes() == y[k].tobytes(), (what, k)


# ---- 1. sequences on one object ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("memory", ms.MEMORIES["wide"])
@pytest.mark.parametrize("name", ["wide", "wide_reversed"])
def test_wide_sequence(ctx, name, memory, monkeypatch):
    """Object 2052 x 20 x 24, one swathe always: a bucket that fills it exactly (nw 65: L.nw == latWords, and the most
    lattice rows the object ever holds, 47 x 39 of a latRowsMax of 49 x 39 -- the allocation counts a swathe's slices as
    cells), then nw 1, nw 65 by cells, nw 2, nw 33 and nw 64 by rows, no surface at all, nw 1 again -- and the same
    eight in reverse on a second object.  The two runs of 32 x 17 x 13 also equal one another byte for byte."""
    obj, steps = ms.SEQUENCES[name]
    _, outs = run_sequence(ctx, obj, steps, memory, monkeypatch)
    first, again = steps.index(ms.WIDE_STEPS[1]), steps.index(ms.WIDE_STEPS[7])
    assert_bytes_equal(outs[first], outs[again], (name, memory))


@pytest.mark.parametrize("memory", ms.MEMORIES["deep"])
def test_deep_sequence(ctx, memory, monkeypatch):
    """Object 67 x 35 x 264 in swathes of 64: five swathes by the sort weld, exactly one swathe by the lattice weld, two
    swathes the second of which is one slice, two slices, the whole object, a small tube, and the sort weld forced on the
    bucket that a moment ago took the lattice weld.  Which weld ran is read off the radix sort's launches."""
    obj, steps = ms.SEQUENCES["deep"]
    run_sequence(ctx, obj, steps, memory, monkeypatch, weld_launches=True)


def test_keys_sequence(ctx, monkeypatch):
    """The object of the k34 key case (260 x 515 x 1040, swathes of 64, mesh memory at the floor): 32-bit keys with the flag
    in bit 31, 34-bit keys, a small lattice-weld bucket (one swathe), 34-bit keys, 32-bit keys -- the uint32_t and uint64_t
    views of one key scratch in alternation."""
    obj, steps = ms.SEQUENCES["keys"]
    for step in dict.fromkeys(steps):
        print("%s: oracle %.2f s" % (step.name, ms.oracle_step_seconds(obj, step, mk.MEMORY)))
    t = time.perf_counter()
    _, outs = run_sequence(ctx, obj, steps, mk.MEMORY, monkeypatch)
    print("keys sequence: %d steps on the device and their comparison in %.1f s" % (len(steps), time.perf_counter() - t))
    assert sum(len(b["triangles"]) for b in outs[1]) > 100
    assert_bytes_equal(outs[1], outs[3], "k34 twice")
    assert_bytes_equal(outs[0], outs[4], "k32 twice")


@pytest.mark.parametrize("memory", ["ample", "tight"])
def test_batches_with_history(ctx, memory, monkeypatch):
    """Three objects of the wide dims through generate_batch three times, the sizes (nw 64 by rows, nw 1, nw 65 by cells)
    rotated by a lane from call to call: every lane of every call equals the oracle's run of that bucket alone, counter
    deltas included.  Then one generate on lane 0's object alone."""
    import mlsgpu_amd as m
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    marchings = [make(ctx, ms.WIDE, memory) for _ in range(3)]
    cnts = [mc.counters() for mc in marchings]
    for rotation in range(3):
        steps = ms.batch_call(rotation)
        gens = [generator(ctx, ms.WIDE, s) for s in steps]
        got = m.Marching.generate_batch(marchings, gens, [s.size for s in steps], [s.key_offset for s in steps])
        assert len(got) == 3
        for k, step in enumerate(steps):
            exp, st = ms.oracle_step(ms.WIDE, step, memory)
            what = (memory, "call", rotation, "lane", k, step)
            assert len(exp) >= 1
            assert_same(got[k], exp, what)
            cnts[k] = assert_counters(marchings[k], st, what, cnts[k])
    check_step(ctx, marchings[0], ms.WIDE, ms.WIDE_STEPS[4], memory, monkeypatch, cnts[0], (memory, "lane 0 alone"))


# ---- 2. undefined padding ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", ms.POISONS)
@pytest.mark.parametrize("name", ["wide", "deep"])
def test_poisoned_padding(ctx, name, poison, monkeypatch):
    """Every step of the wide and the deep sequence with a generator that fills columns [width, pitch) of every row and rows
    [height, zStride) of every slice it writes with NaN, with +-3e38 of alternating sign, or with the field function beyond
    the extent (what processCorners leaves there).  The Generator contract calls that padding undefined; the oracle never
    sees it; the output is the oracle's bit for bit."""
    obj, steps = ms.SEQUENCES[name]
    run_sequence(ctx, obj, steps, "ample", monkeypatch, poison=poison)


@pytest.mark.parametrize("poison", (None,) + ms.POISONS)
def test_padded_object(ctx, poison, monkeypatch):
    """2049 x 17 x 13 and then 33 x 5 x 4 in an object of 2056 x 24 x 24: up to 2023 padding columns and 19 padding rows"""
    obj, steps = ms.SEQUENCES["padded"]
    run_sequence(ctx, obj, steps, "ample", monkeypatch, poison=poison)


# ---- 3. a failed call in the middle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("memory", ["ample", "tight"])
def test_failed_calls(ctx, memory, monkeypatch):
    """On the deep object, after a good bucket: a size one corner beyond the dims in each axis raises LengthError and leaves
    the counters alone; a generator whose callback raises at the second swathe of a bucket of three (at tight memory after
    ship-outs, at ample with the first swathe buffered) is reported as the callback error.  The bucket after each failure
    equals the oracle and its counter deltas count that bucket alone."""
    import mlsgpu_amd as m
    from mlsgpu_amd import binding as mb
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    obj = ms.DEEP
    mc = make(ctx, obj, memory)
    _, cnt = check_step(ctx, mc, obj, ms.DEEP_STEPS[5], memory, monkeypatch, mc.counters(), (memory, "before"))
    for size in ms.BEYOND:
        with pytest.raises(m.binding.LengthError):
            mc.generate(generator(ctx, obj, ms.DEEP_STEPS[0]), size, mx.KEY_OFFSET)
        assert mc.counters() == cnt, size
    _, cnt = check_step(ctx, mc, obj, ms.AFTER_FAILURE[0], memory, monkeypatch, cnt, (memory, "after LengthError"))

    step = ms.FAILING
    gen = ms.PoisonGenerator(ctx, obj, step.fn, "nan", fail_at=2)
    col = mb.MeshCollector(ctx)
    rc = mb.lib().mlsgpu_hip_marching_generate(mc.h, mb.C.byref(gen.struct), col.cb, None, mb._p(mb._u3(step.size)),
                                               mb._p(mb._u3(step.key_offset)))
    ctx.synchronize()
    assert rc == 5                                      # MLSGPU_ERR_CALLBACK, what the callback returned
    with pytest.raises(mb.MlsError):
        mb.check(rc)
    assert isinstance(gen.error, ms.GeneratorFailure) and gen.calls == 2 and gen.blocks == obj.max_swathe
    assert col.error is None
    shipped = mc.counters()["shipouts"] - cnt["shipouts"]
    assert shipped == len(col.batches) and (shipped > 0) == (memory == "tight")
    cnt = mc.counters()
    check_step(ctx, mc, obj, ms.AFTER_FAILURE[1], memory, monkeypatch, cnt, (memory, "after the generator's failure"))


# ---- 4. the worker ------------------------------------------------------------------------------------------------------------

WORKER_COUNTERS = ("shipouts", "occupied", "unwelded", "indices", "welded", "external")


def make_worker(ctx, lanes=None):
    import mlsgpu_amd as m
    cloud = ms.worker_cloud()
    w = m.Worker(ctx, len(cloud), max_cells=63)
    w.set_keep_splats(True)                 # the buckets share one resident cloud: it has to stay as it came
    if lanes:
        w.set_batch(lanes)
    return w, m.DeviceBuffer(ctx, array=cloud), ms.worker_items(len(cloud))


def test_worker_sequence(ctx):
    """One worker of 64 corners a side: the full bucket, (9, 64, 17), (64, 9, 9), a bucket of 0 splats, (33, 33, 33) and the
    full bucket again, each against the whole-bucket oracle's run of it alone, marching counters included."""
    import mlsgpu_amd as m
    w, buf, items = make_worker(ctx)
    for i, item in enumerate(items):
        exp, st, _ = ms.worker_oracle(i)
        before = w.marching_counters()
        got = w.process(buf, *item)
        assert_batches_equal(got, exp)
        assert (len(got) == 0) == (ms.WORKER_SIZES[i] is None), i
        after = w.marching_counters()
        for k in WORKER_COUNTERS:
            assert after[k] - before[k] == st[k], (i, k)
    cloud = ms.worker_cloud()
    np.testing.assert_array_equal(buf.download(m.SPLAT_DTYPE, len(cloud)).view(np.uint32), cloud.view(np.uint32))


def test_worker_batches(ctx):
    """The same six buckets as two process_batch calls of three on one worker of three lanes, in two orders one after the
    other: every lane sees a size unlike its previous one, four times."""
    w, buf, items = make_worker(ctx, lanes=3)
    for order in ms.WORKER_ORDERS:
        for call in order:
            before = w.marching_counters()
            got = w.process_batch(buf, [items[i] for i in call])
            after = w.marching_counters()
            assert len(got) == 3
            total = dict.fromkeys(WORKER_COUNTERS, 0)
            for i, g in zip(call, got):
                exp, st, _ = ms.worker_oracle(i)
                assert_batches_equal(g, exp)
                for k in WORKER_COUNTERS:
                    total[k] += st[k]
            for k in WORKER_COUNTERS:
                assert after[k] - before[k] == total[k], (call, k)
