/*
 * What the stages that work on a finished mesh in HBM share (topology.hip, simplify.hip, normals.hip, smooth.hip, fill.hip,
 * repair.hip; flip.hip, collapse.hip and split.hip through meshedges.hpp; deviation.hip and intersect.hip through meshgrid.hpp):
 * wave-level counting, the records of a triangle's directed sides, the scratch of their sort, and the fixed point that makes
 * a sum independent of the schedule.  Three facts the stages rely on are written here once.
 *
 * Counts are sent once per workgroup.  The atomics of ONE address are served one after the other, about 10 ns apiece: a
 * count or a maximum that every wave of a thread-per-element grid sends there costs 10 ms for the 22 M records of a
 * 4 M-triangle chunk (profiles/NOTES_smooth.md, NOTES_fill.md).  A kernel whose count is hit in most waves therefore runs
 * at most LOOP_BLOCKS workgroups that loop over the elements, add up in registers and LDS (GroupCounts) and send each
 * count once.  tally() -- one atomic per wave -- is for counts that few waves hit (defects), and for topology.hip's
 * kernels, which have not been moved yet.
 *
 * A dead record sorts last.  A directed side from -> to is the key from << b | to, b the bit length of V; the records of a
 * triangle that takes no part (an index >= V, a vertex twice) get from = V, which b bits hold as well.  They sort behind
 * every live record, so the live ones are a prefix that no search leaves, and a kernel over the records drops them by
 * `from >= numVertices` without a flag array.  An index >= V is compared and counted, never used as an address.
 *
 * Non-negative floats order as their bits.  Sign cleared, an IEEE number's exponent field lies above its mantissa, so the
 * largest |x| is an integer maximum over the bit patterns -- which atomicMax has and a float maximum has not -- and a NaN
 * lands above infinity, where the callers' finiteness checks see it.  The same holds for doubles and 64-bit patterns.
 */
#ifndef MLSGPU_AMD_MESHPOST_HPP
#define MLSGPU_AMD_MESHPOST_HPP

#include "common.hpp"
#include "meshgridplan.hpp"      /* bitLength, exponentOfDoubleBits, powerOfTwo: host arithmetic a plain compiler takes too */
#include "primitives.hpp"

namespace mlsgpu
{

typedef unsigned long long Counter;     /* a 64-bit word of a stage's counter block: what atomicAdd / atomicMax take */

/* the most workgroups of a kernel that loops over its elements and sends its counts once (above) */
const uint32_t LOOP_BLOCKS = 1024;

/* ---------------------------------------------------------------- fixed point */

const double CLAMP = 4611686018427387904.0;     /* 2^62: what a value is clamped to before it becomes an integer */

/* e with 2^e <= M < 2^(e + 1) from the bits of a float M >= 0 (a subnormal's true exponent), 0 for M == 0 */
__host__ __device__ inline int exponentOfBits(uint32_t bits)
{
    if (bits == 0)
        return 0;
    const uint32_t field = bits >> 23;
    if (field != 0)
        return (int) field - 127;
    int high = 0;
    while ((bits >> (high + 1)) != 0)
        high++;
    return high - 149;
}

#ifdef __HIPCC__

/* Q of the contracts: x times a power of two (exact: a float times 2^(30 - e) is a normal double or zero), rounded to an
 * integer with ties to even.  The clamp changes no value of a call that is not refused (those are far below 2^62) and makes
 * the conversion of every other one defined: fmax / fmin hand back the bound for a NaN. */
__device__ __forceinline__ long long quantise(float x, double scale)
{
    return (long long) rint(fmin(fmax((double) x * scale, -CLAMP), CLAMP));
}

/* ---------------------------------------------------------------- counting */

/* The lanes of the wave for which `hit` holds add their number to *count with ONE atomic, issued by the ballot's lowest
 * lane.  With `first`, that lane also lowers *first to its `index`: indices rise with the lane, so it holds the lowest. */
__device__ __forceinline__ void tally(bool hit, Counter *count, uint64_t index = 0, Counter *first = nullptr)
{
    const uint64_t mask = __ballot(hit);
    if (hit && popcBelow(mask) == 0)
    {
        atomicAdd(count, (Counter) __popcll(mask));
        if (first != nullptr)
            atomicMin(first, (Counter) index);
    }
}

/* The helpers from here to GroupCounts need the FULL wave: a kernel that calls them keeps every lane to the end. */

/* the sum over the wave, in every lane */
__device__ __forceinline__ long long waveSum64(long long v)
{
#pragma unroll
    for (int step = 1; step < WAVE; step <<= 1)
        v += __shfl_xor(v, step, WAVE);
    return v;
}

/* the largest 64-bit pattern of the wave: the largest high word, then the largest low word among its holders */
__device__ __forceinline__ uint64_t waveMax64(uint64_t bits)
{
    const uint32_t hi = waveMax((uint32_t) (bits >> 32));
    const uint32_t lo = waveMax((uint32_t) (bits >> 32) == hi ? (uint32_t) bits : 0u);
    return (uint64_t) hi << 32 | lo;
}

/* The largest of the wave's bit patterns into *word, for a thread-per-element grid.  The word is read first: a maximum is
 * reached by the first few waves, and the others then have nothing to send (a stale read costs an atomic, never the result). */
__device__ __forceinline__ void foldMax(uint32_t bits, Counter *word)
{
    const uint32_t most = waveMax(bits);
    if (laneId() == 0 && (Counter) most > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(word, (Counter) most);
}

/* The LDS side of "send once": a __shared__ object of a workgroup of at least SUMS + MAXES threads.  clear() first; behind
 * the kernel's loop every wave hands in what its lanes hold in registers; flush() sends each slot that is not zero with one
 * atomic, slot k to counters[at[k]].  A slot is 32 bits: what ONE workgroup counts must fit (the kernels say why it does). */
template<int SUMS, int MAXES = 0>
struct GroupCounts
{
    uint32_t slot[SUMS + MAXES];        /* the sums, then the maxima */

    __device__ __forceinline__ void clear()
    {
        if (threadIdx.x < SUMS + MAXES)
            slot[threadIdx.x] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void add(int k, uint32_t ofLane)
    {
        const uint32_t ofWave = waveSum(ofLane);
        if (laneId() == 0 && ofWave != 0)
            atomicAdd(&slot[k], ofWave);
    }
    __device__ __forceinline__ void raise(int k, uint32_t ofLane)
    {
        const uint32_t ofWave = waveMax(ofLane);
        if (laneId() == 0 && ofWave != 0)
            atomicMax(&slot[SUMS + k], ofWave);
    }
    __device__ __forceinline__ void flush(Counter *counters, const int (&at)[SUMS + MAXES])
    {
        __syncthreads();
        const uint32_t k = threadIdx.x;
        if (k < SUMS + MAXES && slot[k] != 0)
        {
            if (k < SUMS)
                atomicAdd(&counters[at[k]], (Counter) slot[k]);
            else
                atomicMax(&counters[at[k]], (Counter) slot[k]);
        }
    }
};

/* Lanes of a wave that share a root combine before they touch it (a rim of 10^5 vertices hangs on ONE root): body(root,
 * same, sharers, leads) runs once per distinct root among the lanes that are `on`, in every lane of the wave -- `same` in
 * the lanes that hold this root, `sharers` their mask, `leads` in the one that sends for them. */
template<typename Body>
__device__ __forceinline__ void forEachRoot(bool on, uint32_t root, Body body)
{
    const uint32_t lane = laneId();
    uint64_t pending = __ballot(on);
    while (pending != 0)
    {
        const uint32_t leader = (uint32_t) __ffsll((unsigned long long) pending) - 1;
        const uint32_t r = (uint32_t) __shfl((int) root, (int) leader, WAVE);
        const bool same = on && root == r;
        const uint64_t sharers = __ballot(same);
        body(r, same, sharers, lane == leader);
        pending &= ~sharers;
    }
}

/* ---------------------------------------------------------------- side keys and their sorted records */

struct SideKeys
{
    uint64_t numVertices;
    uint32_t b;                 /* bitLength(numVertices): V itself fits, the `from` of a dead record */

    static SideKeys of(uint64_t numVertices) { return SideKeys{numVertices, bitLength(numVertices)}; }
    __device__ __forceinline__ uint64_t keyOf(uint64_t from, uint64_t to) const { return (from << b) | to; }
    __device__ __forceinline__ uint64_t fromOf(uint64_t key) const { return key >> b; }
    __device__ __forceinline__ uint32_t toOf(uint64_t key) const { return (uint32_t) (key & ((uint64_t(1) << b) - 1)); }
    __device__ __forceinline__ uint64_t dead() const { return numVertices << b; }
};

/* Which triangles take no part, as smooth.hip and fill.hip define it: an index >= V wins over a vertex twice.  (topology.hip
 * follows the reference's rotation order instead, where (5, 5, 99) is degenerate: it classifies for itself.) */
struct TriangleDefect
{
    bool outOfRange, degenerate;
    __device__ __forceinline__ bool none() const { return !outOfRange && !degenerate; }
};
__device__ __forceinline__ TriangleDefect defectOf(const uint64_t i[3], uint64_t numVertices)
{
    TriangleDefect d;
    d.outOfRange = i[0] >= numVertices || i[1] >= numVertices || i[2] >= numVertices;
    d.degenerate = !d.outOfRange && (i[0] == i[1] || i[1] == i[2] || i[2] == i[0]);
    return d;
}

/* The sorted records, n < 2^32 of them: those that leave a vertex are one segment, ordered by their other end; equal ones are
 * one run. */
struct Records : SideKeys
{
    const uint64_t *keys;
    uint64_t n;
    const uint32_t *vals;       /* what the stage sorted along (topology.hip: the third vertex), or null */

    __device__ __forceinline__ bool head(uint64_t i, uint64_t key) const { return i == 0 || keys[i - 1] != key; }
    /* the only record of its run: exactly one triangle side is this directed side */
    __device__ __forceinline__ bool single(uint64_t i, uint64_t key) const
    {
        return head(i, key) && (i + 1 == n || keys[i + 1] != key);
    }
    __device__ __forceinline__ bool segmentStart(uint64_t i, uint64_t from) const { return i == 0 || fromOf(keys[i - 1]) != from; }
    __device__ __forceinline__ bool segmentEnd(uint64_t i, uint64_t from) const { return i + 1 == n || fromOf(keys[i + 1]) != from; }
    /* the first record with this key inside [lo, hi), or hi: at most 32 halvings */
    __device__ __forceinline__ uint32_t find(uint32_t lo, uint32_t hi, uint64_t key) const
    {
        const uint32_t end = hi;
        while (lo < hi)
        {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        return lo < end && keys[lo] == key ? lo : end;
    }
    __device__ __forceinline__ bool has(uint64_t key) const { return find(0, (uint32_t) n, key) != (uint32_t) n; }
};

/* ---------------------------------------------------------------- the sort's scratch (host) */

namespace       /* as primitives.hpp's drivers are static: a launch site keeps its stat id per translation unit */
{

/* Both sides of a sort of n records by their 64-bit keys with 32-bit values, and its histogram.  The stage writes keys() (and
 * vals(), unless the sort numbers the records itself: iota); behind sort() the side that does not hold the result is free
 * again, one 64-bit and one 32-bit word per record. */
struct SortScratch
{
    DeviceArray<uint64_t> keysA, keysB;
    DeviceArray<uint32_t> valsA, valsB, hist;
    uint64_t n = 0;
    SortResult<uint64_t> sorted = {nullptr, nullptr};

    int alloc(uint64_t records)
    {
        n = records;
        PROPAGATE(keysA.alloc(n));
        PROPAGATE(keysB.alloc(n));
        PROPAGATE(valsA.alloc(n));
        PROPAGATE(valsB.alloc(n));
        return hist.alloc(sortHistElems(n));
    }
    uint64_t bytes() const { return 2 * keysA.bytes(n) + 2 * valsA.bytes(n) + hist.bytes(sortHistElems(n)); }
    uint64_t *keys() const { return keysA.get(); }
    uint32_t *vals() const { return valsA.get(); }
    /* by from, then to: the 2 b bits of a side key.  (A template only so that a stage that does not sort compiles no sort.) */
    template<typename Key = uint64_t>
    int sort(mlsgpu_ctx *ctx, const char *statName, const SideKeys &K, bool iota, Records *R)
    {
        PROPAGATE(radixSort<Key>(ctx, statName, keysA, valsA, keysB, valsB, n, 2 * K.b, iota, hist, nullptr, &sorted));
        *R = Records{K, sorted.keys, n, sorted.vals};
        return MLSGPU_OK;
    }
    uint64_t *freeKeys() const { return sorted.keys == keysA.get() ? keysB.get() : keysA.get(); }
    uint32_t *freeVals() const { return sorted.vals == valsA.get() ? valsB.get() : valsA.get(); }
};

} // namespace

#endif /* __HIPCC__ */

} // namespace mlsgpu

#endif
