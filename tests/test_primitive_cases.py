"""The numpy references of the scan and the sort (primitive_cases.py) against answers worked out by hand: what the GPU
tests compare the kernels with must itself be right."""
import numpy as np

import primitive_cases as pc


def test_scan_by_hand():
    data = np.array([3, 0, 5, 1, 1, 0, 7, 2, 0, 0, 4, 9], np.uint32)
    prefix, total = pc.exclusive_scan(data, 10)
    assert prefix.dtype == np.uint32 and total.dtype == np.uint32
    np.testing.assert_array_equal(prefix, [10, 13, 13, 18, 19, 20, 20, 27, 29, 29, 29, 33])
    assert total == 42


def test_scan_wraps_modulo_2_32():
    data = np.array([0xFFFFFFFF, 2, 0x80000000, 0x80000000, 5], np.uint32)
    prefix, total = pc.exclusive_scan(data, 0xFFFFFFFE)
    np.testing.assert_array_equal(prefix, [0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF, 0x7FFFFFFF, 0xFFFFFFFF])
    assert total == 4


def test_scan_empty_is_the_seed():
    prefix, total = pc.exclusive_scan(np.zeros(0, np.uint32), 7)
    assert prefix.shape == (0,) and total == 7
    prefix, total = pc.exclusive_scan(np.zeros((0, 3), np.uint32), [1, 2, 3])
    assert prefix.shape == (0, 3)
    np.testing.assert_array_equal(total, [1, 2, 3])


def test_scan_of_triples_goes_column_by_column():
    data = np.array([[1, 10, 0xFFFFFFFF], [2, 20, 1], [3, 30, 1], [4, 40, 0]], np.uint32)
    prefix, total = pc.exclusive_scan(data, [100, 0, 5])
    np.testing.assert_array_equal(prefix, [[100, 0, 5], [101, 10, 4], [103, 30, 5], [106, 60, 6]])
    np.testing.assert_array_equal(total, [110, 100, 6])


def test_sort_is_stable_and_ignores_high_bits():
    #                 0     1     2     3     4     5     6     7     8     9     10    11
    keys = np.array([0x13, 0x21, 0x03, 0xF1, 0x12, 0x33, 0x02, 0x41, 0x10, 0x23, 0x51, 0x00], np.uint32)
    # low 4 bits:     3     1     3     1     2     3     2     1     0     3     1     0
    order = pc.stable_sort_order(keys, 4)
    np.testing.assert_array_equal(order, [8, 11, 1, 3, 7, 10, 4, 6, 0, 2, 5, 9])
    np.testing.assert_array_equal(pc.stable_sort_order(keys, 0), np.arange(12))      # no bits: every key ties
    np.testing.assert_array_equal(pc.stable_sort_order(keys, 32), np.argsort(keys, kind="stable"))


def test_sort_u64_whole_key():
    keys = np.array([1 << 63, 5, (1 << 63) | 1, 5, 0, 1 << 40], np.uint64)
    np.testing.assert_array_equal(pc.stable_sort_order(keys, 64), [4, 1, 3, 5, 0, 2])
    np.testing.assert_array_equal(pc.stable_sort_order(keys, 63), [0, 4, 2, 1, 3, 5])
    assert pc.key_mask(np.uint64, 64) == np.uint64(0xFFFFFFFFFFFFFFFF) and pc.key_mask(np.uint32, 32) == 0xFFFFFFFF


def test_per_pass_follows_the_sorts_split():
    # u32: digits of at most 10 bits; u64: 9
    assert [pc.per_pass(b, 4) for b in (0, 1, 10, 11, 17, 20, 21, 28, 32)] == [1, 1, 10, 6, 9, 10, 7, 10, 8]
    assert [pc.per_pass(b, 8) for b in (9, 10, 43, 63, 64)] == [9, 5, 9, 9, 8]
    assert pc.per_pass(17, 4, max_digit_bits=4) == 4 and pc.per_pass(43, 8, max_digit_bits=4) == 4
    assert pc.per_pass(17, 4, max_digit_bits=10) == 9                    # not narrower than the default: ignored


def test_presorted_input_sorts_to_the_same_answer():
    """What `doneBits` rests on: sorting the keys stably by the remaining bits, after a stable sort by the low bits, is the
    stable sort of the original order by all the bits."""
    keys = np.array([0x13, 0x21, 0x03, 0x31, 0x12, 0x33, 0x02, 0x11, 0x10, 0x23, 0x21, 0x00], np.uint32)
    vals = np.arange(12, dtype=np.uint32)
    k1, v1 = pc.presorted(keys, vals, 4)
    np.testing.assert_array_equal(v1, [8, 11, 1, 3, 7, 10, 4, 6, 0, 2, 5, 9])
    np.testing.assert_array_equal(k1, keys[v1])
    rest = np.argsort(k1 >> np.uint32(4), kind="stable")                 # the passes that are left
    np.testing.assert_array_equal(v1[rest], vals[pc.stable_sort_order(keys, 8)])
    np.testing.assert_array_equal(v1[rest], [11, 6, 2, 8, 7, 4, 0, 1, 10, 9, 3, 5])
