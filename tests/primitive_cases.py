"""Plain numpy references of the device-wide primitives (mlsgpu_amd/csrc/primitives.hpp): exclusive scan with a seed,
modulo 2^32, and stable sort on the low `bits` of the key.  test_primitive_cases.py pins them with hand-written answers;
test_gpu_primitives.py compares the kernels with them word for word."""
import numpy as np

# the widest digit a pass sorts by (SortCaps<K>::MAX_DIGIT_BITS), by key size in bytes
MAX_DIGIT_BITS = {4: 10, 8: 9}


def exclusive_scan(data, seed):
    """(prefix, total) of uint32 `data`, shape (n,) or (n, 3) scanned per column, starting at `seed` (a scalar or one value
    per column): prefix[i] = seed + data[0] + ... + data[i - 1] and total = seed + sum, both modulo 2^32."""
    data = np.asarray(data, dtype=np.uint32)
    seed = np.asarray(seed, dtype=np.uint64)
    incl = np.cumsum(data, axis=0, dtype=np.uint64)
    excl = np.concatenate([np.zeros((1,) + data.shape[1:], np.uint64), incl[:-1]]) if len(data) else incl
    total = (incl[-1] if len(data) else np.zeros(data.shape[1:], np.uint64)) + seed
    return (excl + seed).astype(np.uint32), total.astype(np.uint32)


def key_mask(dtype, bits):
    """The low `bits` bits of a key of `dtype` (bits may be the whole key, or none of it)."""
    return np.dtype(dtype).type((1 << bits) - 1)


def stable_sort_order(keys, bits):
    """The permutation that sorts `keys` stably by their low `bits` bits; whatever lies above them is ignored."""
    keys = np.asarray(keys)
    return np.argsort(keys & key_mask(keys.dtype, bits), kind="stable")


def per_pass(bits, key_bytes, max_digit_bits=None):
    """Digit width of the passes of a sort on `bits` bits, as radixSortBatch splits it: ceil(bits / widest) passes of
    ceil(bits / passes) bits each, the last one narrower if need be.  The only `doneBits` a caller may claim short of
    `bits` itself: the first pass of that split, done elsewhere."""
    widest = MAX_DIGIT_BITS[key_bytes]
    if max_digit_bits is not None and 1 <= max_digit_bits < widest:
        widest = max_digit_bits
    bits = max(bits, 1)
    passes = (bits + widest - 1) // widest
    return (bits + passes - 1) // passes


def presorted(keys, vals, done_bits):
    """(keys, vals) as a sort with `doneBits` receives them: sorted stably by the low `done_bits` bits of the key."""
    order = stable_sort_order(keys, done_bits)
    return keys[order], vals[order]
