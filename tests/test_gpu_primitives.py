"""Scan and radix sort of the HIP path against numpy (clogs::Scan / clogs::Radixsort semantics)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import primitive_cases as pc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


# one launch up to 1024 tiles of 2048 elements, two up to 4096 tiles, three beyond
@pytest.mark.parametrize("n,seed", [(0, 5), (1, 0), (63, 1), (64, 7), (4096, 0), (4097, 3), (1_000_003, 1), (2_097_152, 2),
                                    (2_097_153, 9), (5_000_000, 4), (9_000_001, 6)])
def test_scan_u32(ctx, n, seed):
    import mlsgpu_amd as m
    rng = np.random.RandomState(n + 1)
    data = rng.randint(0, 4, size=n).astype(np.uint32)
    buf = m.DeviceBuffer(ctx, array=data if n else np.zeros(1, np.uint32))
    m.binding.check(m.lib().mlsgpu_hip_test_scan_u32(ctx.h, buf.ptr, n, seed))
    got = buf.download(np.uint32, n)
    exp = (np.concatenate([[0], np.cumsum(data[:-1], dtype=np.uint64)]) + seed).astype(np.uint32) if n else data
    np.testing.assert_array_equal(got, exp)


def test_scan_launches_back_to_back(ctx):
    """The one-launch scan's flags are never cleared (a launch's flags carry its epoch): scans of changing sizes, one
    behind the other on one stream, each see only their own."""
    import mlsgpu_amd as m
    rng = np.random.RandomState(77)
    sizes = [int(x) for x in rng.randint(1, 600_000, size=40)] + [2_097_152, 5, 2_000_000, 2049, 2048, 1]
    bufs, datas = [], []
    for n in sizes:
        data = rng.randint(0, 5, size=n).astype(np.uint32)
        datas.append(data)
        bufs.append(m.DeviceBuffer(ctx, array=data))
    for rep in range(3):
        for k, (n, buf) in enumerate(zip(sizes, bufs)):
            if rep:
                buf.upload(datas[k])
            m.binding.check(m.lib().mlsgpu_hip_test_scan_u32(ctx.h, buf.ptr, n, k))
        for k, (n, buf) in enumerate(zip(sizes, bufs)):
            exp = (np.concatenate([[0], np.cumsum(datas[k][:-1], dtype=np.uint64)]) + k).astype(np.uint32)
            np.testing.assert_array_equal(buf.download(np.uint32, n), exp)


def _scan_batch(m, ctx, ins, outs, sizes, seeds, repeats):
    k = len(ins)
    pin = (C.c_void_p * k)(*[b.ptr for b in ins])
    pout = (C.c_void_p * k)(*[b.ptr for b in outs])
    pn = (C.c_uint64 * k)(*sizes)
    ps = (C.c_uint32 * k)(*seeds)
    m.binding.check(m.lib().mlsgpu_hip_test_scan_u32_batch(ctx.h, pin, pout, pn, ps, k, repeats))


def test_scan_batch_lanes(ctx):
    """A batch's scans: one set of launches for up to eight lanes of different lengths (an empty lane among them)."""
    import mlsgpu_amd as m
    rng = np.random.RandomState(3)
    sizes = [2_097_152, 1, 0, 777_777, 2048, 2049, 1_500_000, 63]
    datas = [rng.randint(0, 4, size=max(n, 1)).astype(np.uint32) for n in sizes]
    ins = [m.DeviceBuffer(ctx, array=d) for d in datas]
    outs = [m.DeviceBuffer(ctx, array=np.full(max(n, 1), 0xDEAD, np.uint32)) for n in sizes]
    seeds = list(range(10, 18))
    _scan_batch(m, ctx, ins, outs, sizes, seeds, 3)
    for n, d, o, sd in zip(sizes, datas, outs, seeds):
        if n:
            exp = (np.concatenate([[0], np.cumsum(d[:n - 1], dtype=np.uint64)]) + sd).astype(np.uint32)
            np.testing.assert_array_equal(o.download(np.uint32, n), exp)


def test_scan_one_launch_under_contention(ctx):
    """The shape bench.py runs: eight lanes x 1024 tiles per launch (four times the workgroups the chip holds), launches
    back to back, while a second context's worker keeps the CUs busy with processCorners on a cfg2-sized bucket.  A
    workgroup's tile is a ticket it draws when it starts, so nothing it waits for can be un-dispatched (VERDICT round 5:
    the scan used blockIdx.x, which is only safe if workgroups are dispatched in order).  A watchdog ends the process with
    its own exit code if a scan call does not return in 10 s -- a hung stream cannot be recovered from inside."""
    import os
    import threading
    import time
    import mlsgpu_amd as m
    from mlsgpu_amd import synth
    lanes, n = 8, 1024 * 2048
    rng = np.random.RandomState(11)
    datas = [rng.randint(0, 3, size=n).astype(np.uint32) for _ in range(lanes)]
    ins = [m.DeviceBuffer(ctx, array=d) for d in datas]
    outs = [m.DeviceBuffer(ctx, array=np.zeros(n, np.uint32)) for _ in range(lanes)]
    seeds = [7 * k for k in range(lanes)]

    cloud, g = synth.make_cloud("cfg2", scale=0.4)
    ctx2 = m.Context(0)
    w = m.Worker(ctx2, len(cloud), max_cells=255)
    w.set_keep_splats(True)
    buf = m.DeviceBuffer(ctx2, array=cloud)
    stop = threading.Event()
    passes = [0]
    errors = []

    def hog():
        try:
            col = m.binding.ChecksumCollector(ctx2)
            while not stop.is_set():
                w.process(buf, 0, len(cloud), (0, 0, 0), (g, g, g), collector=col)
                passes[0] += 1
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    deadline = [None]

    def watchdog():
        while not stop.is_set():
            d = deadline[0]
            if d is not None and time.time() > d:
                os.write(2, b"test_scan_one_launch_under_contention: a scan did not return in 10 s (hung stream)\n")
                os._exit(97)
            time.sleep(0.05)

    th = threading.Thread(target=hog)
    wd = threading.Thread(target=watchdog, daemon=True)
    th.start()
    wd.start()
    try:
        t0 = time.time()
        calls = 0
        while calls < 30 or (passes[0] < 2 and time.time() - t0 < 60):
            deadline[0] = time.time() + 10.0
            _scan_batch(m, ctx, ins, outs, [n] * lanes, seeds, 20)
            deadline[0] = None
            calls += 1
    finally:
        stop.set()
        th.join()
    assert not errors, errors
    assert passes[0] >= 1                                     # the other context really ran beside the scans
    for d, o, sd in zip(datas, outs, seeds):
        exp = (np.concatenate([[0], np.cumsum(d[:-1], dtype=np.uint64)]) + sd).astype(np.uint32)
        np.testing.assert_array_equal(o.download(np.uint32, n), exp)
    del w, buf


@pytest.mark.parametrize("n,bits", [(1, 17), (1000, 1), (4096, 8), (5000, 10), (70_001, 17), (300_000, 28), (300_000, 32)])
def test_sort_u32_stable(ctx, n, bits):
    import mlsgpu_amd as m
    rng = np.random.RandomState(bits * 7 + n % 97)
    keys = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    if bits == 17:
        keys[rng.rand(n) < 0.3] = 0xFFFFFFFF       # the octree's "no entry" keys must sort last
        keys[keys != 0xFFFFFFFF] &= 0x7FFF
    vals = np.arange(n, dtype=np.uint32)
    kb = m.DeviceBuffer(ctx, array=keys)
    vb = m.DeviceBuffer(ctx, array=vals)
    m.binding.check(m.lib().mlsgpu_hip_test_sort_u32(ctx.h, kb.ptr, vb.ptr, n, bits))
    mask = np.uint32((1 << bits) - 1) if bits < 32 else np.uint32(0xFFFFFFFF)
    order = np.argsort(keys & mask, kind="stable")
    np.testing.assert_array_equal(kb.download(np.uint32, n), keys[order])
    np.testing.assert_array_equal(vb.download(np.uint32, n), vals[order])


@pytest.mark.parametrize("n,bits", [(10, 43), (123_457, 43), (50_000, 64)])
def test_sort_u64_stable(ctx, n, bits):
    import mlsgpu_amd as m
    rng = np.random.RandomState(bits + n % 11)
    keys = rng.randint(0, 2 ** 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.randint(0, 2, size=n).astype(np.uint64)
    keys[: n // 3] = keys[n // 3: 2 * (n // 3)]      # duplicates exercise stability
    vals = np.arange(n, dtype=np.uint32)
    kb = m.DeviceBuffer(ctx, array=keys)
    vb = m.DeviceBuffer(ctx, array=vals)
    m.binding.check(m.lib().mlsgpu_hip_test_sort_u64(ctx.h, kb.ptr, vb.ptr, n, bits))
    mask = np.uint64((1 << bits) - 1) if bits < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    order = np.argsort(keys & mask, kind="stable")
    np.testing.assert_array_equal(kb.download(np.uint64, n), keys[order])
    np.testing.assert_array_equal(vb.download(np.uint32, n), vals[order])


# ---------------------------------------------------------------------------------------------------------------------
# Scan and sort under the options their callers use (mlsgpu_hip_test_scan / mlsgpu_hip_test_sort_batch).  Every buffer a
# primitive is handed has GUARD_WORDS words of GUARD behind its n elements, which must come back untouched; output arrays
# start out as FILL, which must survive wherever the primitive has no business writing.

GUARD_WORDS = 64
GUARD = 0x6A6A9595
FILL = 0xDEADBEEF
MAX_BATCH = 8                   # MLSGPU_MAX_BATCH
SCAN_KINDS = [1, 3]             # words per element: uint32, U3
SCAN_FORMS = {"whole": 0, "two_inputs": 1, "phases": 2}         # MLSGPU_TEST_SCAN_*
SCAN_SEED = np.array([0xFFFFFF00, 7, 0x80000001], np.uint32)
SCAN_SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 5 * 2048 + 1, 300 * 2048 + 777]
SCAN_CAPACITY = 5 * 2048 + 1
SCAN_COUNTS = [0, 1, 2048, 2049, SCAN_CAPACITY - 1, SCAN_CAPACITY, SCAN_CAPACITY + 5]
SORT_KEYS = {4: np.uint32, 8: np.uint64}
SORT_OPTION_CASES = [(4, 17, 9_001), (4, 17, 70_001), (8, 43, 9_001), (8, 43, 70_001)]
SORT_CAPACITY = 3 * 4096 + 5
SORT_COUNTS = [0, 1, 4095, 4096, 4097, SORT_CAPACITY - 1, SORT_CAPACITY, SORT_CAPACITY + 5]
SORT_LANE_SIZES = [70_001, 1, 0, 4096, 4097, 12_293, 63, 300_000]
SORT_BIG_SIZES = [256 * 4096 + 4097, 600 * 4096 - 17]


class Guarded:
    """A device buffer of `payload` followed by the guard band."""

    def __init__(self, ctx, payload):
        import mlsgpu_amd as m
        payload = np.ascontiguousarray(payload)
        self.nbytes = payload.nbytes
        raw = np.concatenate([payload.reshape(-1).view(np.uint32), np.full(GUARD_WORDS, GUARD, np.uint32)])
        self.buf = m.DeviceBuffer(ctx, array=raw)
        self.ptr = self.buf.ptr

    def get(self, dtype):
        return self.buf.download(dtype, self.nbytes // np.dtype(dtype).itemsize)

    def assert_guard_intact(self, what):
        guard = self.buf.download(np.uint32, GUARD_WORDS, offset=self.nbytes)
        np.testing.assert_array_equal(guard, np.full(GUARD_WORDS, GUARD, np.uint32), err_msg="guard band behind " + what)


def _device_word(ctx, value):
    import mlsgpu_amd as m
    return None if value is None else m.DeviceBuffer(ctx, array=np.array([value], np.uint32))


@functools.lru_cache(maxsize=None)
def scan_input(words, n):
    """Full-range words, so that the sums wrap; the three columns of a triple differ visibly (full range, 0..3, below 2^20)."""
    rng = np.random.RandomState(1000 * words + n % 997)
    data = rng.randint(0, 2 ** 32, size=(n, words), dtype=np.uint64).astype(np.uint32)
    if words == 3:
        data[:, 1] &= 3
        data[:, 2] &= 0xFFFFF
    data = data.reshape(n) if words == 1 else data
    data.setflags(write=False)
    return data


@functools.lru_cache(maxsize=None)
def scan_expected(words, n, live):
    prefix, total = pc.exclusive_scan(scan_input(words, n)[:live], SCAN_SEED[0] if words == 1 else SCAN_SEED)
    prefix.setflags(write=False)
    return prefix, total


def run_scan(ctx, words, form, n, count=None):
    """One scan of scan_input(words, n) in the given form, of which only `count` elements exist if that is given, compared
    with the reference: prefixes, the values the consumer was handed, the total, and everything that must stay untouched."""
    import mlsgpu_amd as m
    data = scan_input(words, n)
    live = n if count is None else min(n, count)
    shape = data.shape
    d_in = Guarded(ctx, data)
    d_prefix = Guarded(ctx, np.full(shape, FILL, np.uint32))
    d_values = Guarded(ctx, np.full(shape, FILL, np.uint32))
    d_total = Guarded(ctx, np.full(words, FILL, np.uint32))
    d_count = _device_word(ctx, count)
    m.binding.check(m.lib().mlsgpu_hip_test_scan(ctx.h, words, SCAN_FORMS[form], d_in.ptr, d_prefix.ptr, d_values.ptr, n,
                                                 SCAN_SEED.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 None if d_count is None else d_count.ptr, d_total.ptr))
    exp_prefix, exp_total = scan_expected(words, n, live)
    prefix = d_prefix.get(np.uint32).reshape(shape)
    values = d_values.get(np.uint32).reshape(shape)
    np.testing.assert_array_equal(d_total.get(np.uint32), np.atleast_1d(exp_total), err_msg="total")
    np.testing.assert_array_equal(prefix[:live], exp_prefix, err_msg="prefix")
    np.testing.assert_array_equal(values[:live], data[:live], err_msg="value handed to the consumer")
    assert (prefix[live:] == FILL).all() and (values[live:] == FILL).all(), "written at or behind min(n, *nDev)"
    np.testing.assert_array_equal(d_in.get(np.uint32).reshape(shape), data, err_msg="input")
    for what, b in (("the input", d_in), ("the prefixes", d_prefix), ("the values", d_values), ("the total", d_total)):
        b.assert_guard_intact(what)


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("form", sorted(SCAN_FORMS))
@pytest.mark.parametrize("words", SCAN_KINDS)
def test_scan_forms(ctx, words, form, n):
    """uint32 and U3, in each of the three forms (the form, not the size, selects the kernels): sizes around a wave, around a
    tile, several tiles, and more than 256 tiles, where the single-workgroup scan of the tile sums and the loop over the
    predecessors' sums go round twice."""
    run_scan(ctx, words, form, n)


@pytest.mark.parametrize("count", SCAN_COUNTS)
@pytest.mark.parametrize("form", sorted(SCAN_FORMS))
@pytest.mark.parametrize("words", SCAN_KINDS)
def test_scan_device_count(ctx, words, form, count):
    """The element count lives on the device: nothing, one element, a tile boundary and one past it, capacity - 1, capacity,
    and more than the capacity (which is clamped).  The total is that of the elements that exist."""
    run_scan(ctx, words, form, SCAN_CAPACITY, count)


@functools.lru_cache(maxsize=None)
def sort_input(key_bytes, n, salt=0):
    """(keys, values): keys random in every bit, a third of them copies of another third (ties in every width); values
    random too, so that they cannot be mistaken for positions."""
    rng = np.random.RandomState(key_bytes * 131 + n % 1009 + 7 * salt)
    keys = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64)
    if key_bytes == 8:
        keys = keys << np.uint64(32) | rng.randint(0, 2 ** 32, size=n, dtype=np.uint64)
    keys = keys.astype(SORT_KEYS[key_bytes])
    keys[: n // 3] = keys[n // 3: 2 * (n // 3)]
    vals = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    vals[vals == FILL] = 0
    keys.setflags(write=False)
    vals.setflags(write=False)
    return keys, vals


def run_sort(ctx, key_bytes, lanes, bits, iota=False, done_bits=0, keys_wanted=True, presort=True):
    """One batched sort.  lanes: (keys, values, count or None) each, in the ORIGINAL order -- with done_bits the device gets
    them sorted stably by those low bits, and the answer is still the stable sort of the original order by all `bits`
    (presort=False: the device gets them as they are, and the answer is their stable sort by bits [done_bits, bits) alone).
    Checks every lane's first min(n, count) results against the reference, the guard bands, and that an empty lane stays as
    it was; returns the sides the lanes' results were reported on."""
    import mlsgpu_amd as m
    dtype = SORT_KEYS[key_bytes]
    k = len(lanes)
    given, bufs = [], []
    for keys, vals, count in lanes:
        n = len(keys)
        assert not (done_bits and count is not None)            # a prefix of the presorted input is another input
        if iota:
            vals = np.full(n, FILL, np.uint32)                  # never read: must not show up in the output
        kin, vin = pc.presorted(keys, vals, done_bits) if done_bits and presort else (keys, vals)
        given.append((keys, vals, kin))
        bufs.append(dict(keys=Guarded(ctx, kin), vals=Guarded(ctx, vin),
                         keys_out=Guarded(ctx, np.full(n * (key_bytes // 4), FILL, np.uint32)),
                         vals_out=Guarded(ctx, np.full(n, FILL, np.uint32)), count=_device_word(ctx, count)))
    ptrs = lambda name: (C.c_void_p * k)(*[None if b[name] is None else b[name].ptr for b in bufs])     # noqa: E731
    sides = (C.c_uint32 * k)(*([99] * k))
    m.binding.check(m.lib().mlsgpu_hip_test_sort_batch(
        ctx.h, key_bytes, k, ptrs("keys"), ptrs("vals"), (C.c_uint64 * k)(*[len(lane[0]) for lane in lanes]), ptrs("count"),
        bits, int(iota), done_bits, int(keys_wanted), ptrs("keys_out"), ptrs("vals_out"), sides))
    for lane, ((_, _, count), (keys, vals, kin), b) in enumerate(zip(lanes, given, bufs)):
        n = len(keys)
        live = n if count is None else min(n, count)
        assert sides[lane] in (0, 1), (lane, sides[lane])
        for name in ("keys", "vals", "keys_out", "vals_out"):
            b[name].assert_guard_intact("lane %d's %s" % (lane, name))
        if n == 0:
            continue                                            # nothing but guard band, and that is intact
        if presort:
            order = pc.stable_sort_order(keys[:live], bits)
            # iota's values are positions in what the device received
            exp_vals = pc.stable_sort_order(kin[:live], bits).astype(np.uint32) if iota else vals[:live][order]
        else:
            order = pc.stable_sort_order(keys[:live] >> dtype(done_bits % (8 * key_bytes)), bits - done_bits)
            exp_vals = order.astype(np.uint32) if iota else vals[:live][order]
        np.testing.assert_array_equal(b["vals_out"].get(np.uint32)[:live], exp_vals, err_msg="lane %d values" % lane)
        got_keys = b["keys_out"].get(dtype)
        if keys_wanted:
            np.testing.assert_array_equal(got_keys[:live], keys[:live][order], err_msg="lane %d keys" % lane)
        else:
            assert (got_keys.view(np.uint32) == FILL).all(), "keys delivered though not wanted"
    return list(sides)


@pytest.mark.parametrize("key_bytes,bits", [(4, b) for b in range(1, 33)] + [(8, b) for b in range(1, 65)])
def test_sort_every_width(ctx, key_bytes, bits):
    """The width decides the number of passes, the digit of each, a narrower last digit, which scatter kernel runs and the
    side the result ends on.  Three tiles, the last one ragged; the bits above `bits` are random and must be ignored."""
    keys, vals = sort_input(key_bytes, 9_001)
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits)


@pytest.mark.parametrize("key_bytes,bits", [(4, 1), (4, 4), (4, 5), (4, 17), (4, 32), (8, 9), (8, 43), (8, 64)])
def test_sort_narrow_digits(ctx, monkeypatch, key_bytes, bits):
    """MLSGPU_HIP_SORT_DIGIT_BITS=4 (read by every call): the same answers from many narrow passes."""
    monkeypatch.setenv("MLSGPU_HIP_SORT_DIGIT_BITS", "4")
    keys, vals = sort_input(key_bytes, 9_001)
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits)
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits, iota=True, done_bits=pc.per_pass(bits, key_bytes, 4) if bits > 4 else 0)


@pytest.mark.parametrize("key_bytes,bits,n", SORT_OPTION_CASES)
def test_sort_iota(ctx, key_bytes, bits, n):
    """iota: the values are the positions, and what valsA holds is never read."""
    keys, vals = sort_input(key_bytes, n)
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits, iota=True)


@pytest.mark.parametrize("key_bytes,bits,n", SORT_OPTION_CASES)
def test_sort_values_only(ctx, key_bytes, bits, n):
    """keysWanted = false: the last pass leaves the keys unwritten, the values arrive all the same."""
    keys, vals = sort_input(key_bytes, n)
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits, keys_wanted=False)
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits, iota=True, keys_wanted=False)


@pytest.mark.parametrize("key_bytes,bits,n", SORT_OPTION_CASES)
def test_sort_done_bits(ctx, key_bytes, bits, n):
    """doneBits = the first pass of the sort's own split, done by someone else: the remaining passes finish the sort.  They do
    not look at the low bits again: keys that are NOT sorted by them come out ordered by bits [doneBits, bits) alone."""
    keys, vals = sort_input(key_bytes, n)
    done = pc.per_pass(bits, key_bytes)
    assert 0 < done < bits
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits, done_bits=done)
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits, done_bits=done, keys_wanted=False)
    run_sort(ctx, key_bytes, [(keys, vals, None)], bits, done_bits=done, presort=False)


@pytest.mark.parametrize("key_bytes,bits,n", SORT_OPTION_CASES)
def test_sort_nothing_left(ctx, key_bytes, bits, n):
    """doneBits == bits: no pass runs and the input is the result, on the side it came in on -- sorted, or not sorted at all."""
    keys, vals = sort_input(key_bytes, n)
    assert run_sort(ctx, key_bytes, [(keys, vals, None)], bits, done_bits=bits) == [0]
    assert run_sort(ctx, key_bytes, [(keys, vals, None)], bits, done_bits=bits, presort=False) == [0]


@pytest.mark.parametrize("key_bytes,n", [(key_bytes, n) for key_bytes, _, n in SORT_OPTION_CASES])
def test_sort_no_bits(ctx, key_bytes, n):
    """bits == 0 (simplify, when every vertex lies in cell 0): one pass still runs, so that iota's values exist."""
    keys = np.zeros(n, SORT_KEYS[key_bytes])
    run_sort(ctx, key_bytes, [(keys, np.zeros(n, np.uint32), None)], 0, iota=True)


@pytest.mark.parametrize("key_bytes,bits,n", SORT_OPTION_CASES)
def test_sort_options_combined(ctx, key_bytes, bits, n):
    """iota with a count on the device (simplify's survivors), and doneBits over several lanes (the octree)."""
    keys, vals = sort_input(key_bytes, n)
    run_sort(ctx, key_bytes, [(keys, vals, n - 4097)], bits, iota=True)
    lanes = [(keys, vals, None), sort_input(key_bytes, 4097, 1) + (None,), sort_input(key_bytes, 63, 2) + (None,)]
    run_sort(ctx, key_bytes, lanes, bits, done_bits=pc.per_pass(bits, key_bytes))


@pytest.mark.parametrize("count", SORT_COUNTS)
@pytest.mark.parametrize("key_bytes,bits", [(4, 17), (8, 43)])
def test_sort_device_count(ctx, key_bytes, bits, count):
    """The element count lives on the device: nothing, one element, a tile boundary and its neighbours, capacity - 1,
    capacity, and more than the capacity (which is clamped).  The first min(n, count) results are defined."""
    keys, vals = sort_input(key_bytes, SORT_CAPACITY)
    run_sort(ctx, key_bytes, [(keys, vals, count)], bits)


@pytest.mark.parametrize("key_bytes,bits", [(4, 17), (8, 43)])
def test_sort_batch_lanes(ctx, key_bytes, bits):
    """As many lanes as a batch may have, of different lengths, in one call; one of them with a device count below its n,
    one of them empty: that one is not written to and still reports a side."""
    assert len(SORT_LANE_SIZES) == MAX_BATCH
    lanes = [sort_input(key_bytes, n, lane) + (5_000 if n == 12_293 else None,) for lane, n in enumerate(SORT_LANE_SIZES)]
    run_sort(ctx, key_bytes, lanes, bits)
    run_sort(ctx, key_bytes, lanes, bits, iota=True, keys_wanted=False)


@pytest.mark.parametrize("n", SORT_BIG_SIZES)
@pytest.mark.parametrize("key_bytes", [4, 8])
def test_sort_remapped_tiles(ctx, key_bytes, n):
    """256 sort tiles or more: the histogram and scatter kernels deal tiles to workgroups in runs of 32 (tileOfWorkgroup),
    whole groups of 256 that way and the rest as they come.  Below 256 tiles the mapping is the identity."""
    keys, _ = sort_input(key_bytes, n)
    run_sort(ctx, key_bytes, [(keys, None, None)], 8 * key_bytes, iota=True)


def test_sort_remapped_tiles_device_count(ctx):
    """The same with a count on the device that ends inside an earlier tile."""
    n = SORT_BIG_SIZES[0]
    keys, _ = sort_input(8, n)
    run_sort(ctx, 8, [(keys, None, n - 4097)], 64, iota=True)


# ---------------------------------------------------------------------------------------------------------------------
# The two documented fallback routes.  Each is read once per process, so each runs in a fresh child.

TESTS = os.path.dirname(os.path.abspath(__file__))


def _cases(module, name):
    """(node id, number of test cases) of a test function with all its parameter sets."""
    count = 1
    for mark in getattr(getattr(module, name), "pytestmark", []):
        if mark.name == "parametrize":
            count *= len(mark.args[1])
    return os.path.join(TESTS, module.__name__ + ".py") + "::" + name, count


def run_route(variable, selection):
    """The selected tests in ONE fresh pytest process with `variable`=0: all of them must run and pass."""
    env = dict(os.environ)
    env[variable] = "0"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "pytest", "-q", "-x", "-m", "gpu",
                                                                            "-p", "no:cacheprovider"]
    done = subprocess.run(cmd + [node for node, _ in selection], cwd=os.path.dirname(TESTS), env=env, timeout=900,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    tail = "\n".join(done.stdout.splitlines()[-25:])
    assert done.returncode == 0, "%s=0: exit status %d\n%s" % (variable, done.returncode, tail)
    summary = [line for line in done.stdout.splitlines() if re.search(r"\b\d+ passed\b", line)]
    assert summary, tail
    counts = dict((what, int(num)) for num, what in re.findall(r"(\d+) (passed|failed|skipped|deselected|errors?|xfailed|xpassed)",
                                                               summary[-1]))
    assert counts == {"passed": sum(c for _, c in selection)}, summary[-1]


def test_route_without_one_launch_scan():
    """MLSGPU_HIP_SCAN_ONEPASS=0: every scan in its two- or three-launch form -- the scan tests of this file, the octree at
    every depth, on saturated tiles and on a batch of mixed lanes, and one Marching volume."""
    import test_gpu_marching
    import test_gpu_tree
    me = sys.modules[__name__]
    selection = [_cases(me, name) for name in ("test_scan_u32", "test_scan_launches_back_to_back", "test_scan_batch_lanes",
                                               "test_scan_one_launch_under_contention", "test_scan_forms",
                                               "test_scan_device_count")]
    selection += [_cases(test_gpu_tree, name) for name in ("test_every_tree_depth", "test_saturated_tiles",
                                                           "test_build_batch_mixed_lanes")]
    assert "tsphere" in test_gpu_marching.GENERATE_CASES
    selection.append((_cases(test_gpu_marching, "test_generate_manifold_and_parity")[0] + "[tsphere]", 1))
    run_route("MLSGPU_HIP_SCAN_ONEPASS", selection)


def test_route_without_fused_octree_pass():
    """MLSGPU_HIP_OCTREE_FUSED=0: the octree's entries sorted by the generic radix sort -- every depth, the default geometry,
    saturated tiles, skewed keys, the grid's faces, and the worker on trees that are not the default."""
    import test_gpu_fp64
    import test_gpu_tree
    selection = [_cases(test_gpu_tree, "test_every_tree_depth"), _cases(test_gpu_tree, "test_parity_default_geometry"),
                 _cases(test_gpu_fp64, "test_worker_non_default_tree")]
    selection += [_cases(test_gpu_tree, name) for name in ("test_saturated_tiles", "test_skewed_keys", "test_grid_faces")]
    run_route("MLSGPU_HIP_OCTREE_FUSED", selection)
