/*
 * Test entry points of the device-wide primitives (primitives.hpp): the scan and the radix sort with every option
 * their callers use, reachable from the suite without an octree, a bucket or a mesh around them.  Each entry point
 * returns when its work on the context's stream has finished.
 */
#include "common.hpp"
#include "primitives.hpp"

#include <cstring>
#include <vector>

using namespace mlsgpu;

MLSGPU_API int mlsgpu_hip_test_scan_u32(mlsgpu_ctx *ctx, uint32_t *dData, uint64_t n, uint32_t seed)
{
    REQUIRE(ctx != nullptr, MLSGPU_ERR_INVALID);
    HIP_CHECK(hipSetDevice(ctx->device));
    DeviceArray<uint32_t> dTiles;
    PROPAGATE(dTiles.alloc((uint64_t) scanTiles(n) + 1));
    int rc = exclusiveScan<uint32_t>(ctx, "test.scan", ArrayIn<uint32_t>{dData}, ArrayOut<uint32_t>{dData}, n, seed,
                                     dTiles.get(), (uint32_t *) nullptr);
    hipStreamSynchronize(ctx->stream);
    return rc;
}

/* `repeats` scans of `count` lanes each (one set of launches per repeat, as the buckets of a batch), dIn[k] -> dOut[k],
 * enqueued back to back without a host synchronisation in between; returns when the last one has finished */
MLSGPU_API int mlsgpu_hip_test_scan_u32_batch(mlsgpu_ctx *ctx, const uint32_t *const *dIn, uint32_t *const *dOut, const uint64_t *n,
                                              const uint32_t *seeds, uint32_t count, uint32_t repeats)
{
    REQUIRE(ctx != nullptr && dIn != nullptr && dOut != nullptr && n != nullptr && seeds != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(count >= 1 && count <= MAX_LANES, MLSGPU_ERR_LENGTH);
    HIP_CHECK(hipSetDevice(ctx->device));
    DeviceArray<uint32_t> dTiles[MAX_LANES];
    typedef ScanJob<uint32_t, ArrayIn<uint32_t>, ArrayIn<uint32_t>, ArrayOut<uint32_t> > Job;
    Job jobs[MAX_LANES];
    int rc = MLSGPU_OK;
    for (uint32_t k = 0; k < count && rc == MLSGPU_OK; k++)
    {
        rc = dTiles[k].alloc((uint64_t) scanTiles(n[k]) + 1);
        jobs[k] = Job{ArrayIn<uint32_t>{dIn[k]}, ArrayIn<uint32_t>{dIn[k]}, ArrayOut<uint32_t>{dOut[k]}, n[k], seeds[k], dTiles[k],
                      (uint32_t *) nullptr, (const uint32_t *) nullptr};
    }
    for (uint32_t r = 0; r < repeats && rc == MLSGPU_OK; r++)
        rc = exclusiveScanBatch<uint32_t>(ctx, "test.scan", jobs, count);
    hipStreamSynchronize(ctx->stream);
    return rc;
}

template<typename K>
static int testSort(mlsgpu_ctx *ctx, K *dKeys, uint32_t *dValues, uint64_t n, uint32_t bits)
{
    HIP_CHECK(hipSetDevice(ctx->device));
    DeviceArray<K> kb;
    DeviceArray<uint32_t> vb, hist, tiles;
    PROPAGATE(kb.alloc(n + 1));
    PROPAGATE(vb.alloc(n + 1));
    PROPAGATE(hist.alloc(sortHistElems(n) + 1));
    PROPAGATE(tiles.alloc((uint64_t) scanTiles(sortHistElems(n)) + 1));
    SortResult<K> res;
    int rc = radixSort<K>(ctx, "test.sort", dKeys, dValues, kb, vb, n, bits, false, hist, tiles, &res);
    if (rc == MLSGPU_OK && res.keys != dKeys && n > 0)
    {
        hipMemcpyAsync(dKeys, res.keys, n * sizeof(K), hipMemcpyDeviceToDevice, ctx->stream);
        hipMemcpyAsync(dValues, res.vals, n * 4, hipMemcpyDeviceToDevice, ctx->stream);
    }
    hipStreamSynchronize(ctx->stream);
    return rc;
}

MLSGPU_API int mlsgpu_hip_test_sort_u32(mlsgpu_ctx *ctx, uint32_t *dKeys, uint32_t *dValues, uint64_t n, uint32_t bits)
{
    REQUIRE(ctx != nullptr, MLSGPU_ERR_INVALID);
    return testSort<uint32_t>(ctx, dKeys, dValues, n, bits);
}

MLSGPU_API int mlsgpu_hip_test_sort_u64(mlsgpu_ctx *ctx, uint64_t *dKeys, uint32_t *dValues, uint64_t n, uint32_t bits)
{
    REQUIRE(ctx != nullptr, MLSGPU_ERR_INVALID);
    return testSort<uint64_t>(ctx, dKeys, dValues, n, bits);
}

/* ---- the scan, by element kind and form ---- */

namespace
{

/* two functor types that compute the same value: exclusiveScan2 takes the one-launch form only where In1 and In2 are one type */
template<typename T>
struct FirstIn
{
    const T *p;
    __device__ __forceinline__ T operator()(uint64_t i) const { return p[i]; }
};
template<typename T>
struct SecondIn
{
    const T *p;
    __device__ __forceinline__ T operator()(uint64_t i) const { return p[i]; }
};
/* keeps both things a consumer is handed */
template<typename T>
struct BothOut
{
    T *prefix, *values;
    __device__ __forceinline__ void operator()(uint64_t i, T excl, T v) const
    {
        prefix[i] = excl;
        values[i] = v;
    }
};

uint32_t makeSeed(const uint32_t *s, uint32_t) { return s[0]; }
U3 makeSeed(const uint32_t *s, U3) { return U3{s[0], s[1], s[2]}; }

template<typename T>
int testScan(mlsgpu_ctx *ctx, uint32_t form, const void *dIn, void *dPrefix, void *dValues, uint64_t n, const uint32_t *seedWords,
             const uint32_t *nDev, void *dTotal)
{
    DeviceArray<T> dTiles;
    PROPAGATE(dTiles.alloc((uint64_t) scanTiles(n) + 1));
    const T seed = makeSeed(seedWords, T());
    const T *const in = (const T *) dIn;
    const BothOut<T> out{(T *) dPrefix, (T *) dValues};
    T *const total = (T *) dTotal;
    int rc;
    if (form == MLSGPU_TEST_SCAN_WHOLE)
        rc = exclusiveScan<T>(ctx, "test.scan", FirstIn<T>{in}, out, n, seed, dTiles.get(), total, nDev);
    else if (form == MLSGPU_TEST_SCAN_TWO_INPUTS)
        rc = exclusiveScan2<T>(ctx, "test.scan", FirstIn<T>{in}, SecondIn<T>{in}, out, n, seed, dTiles.get(), total, nDev);
    else
    {
        rc = scanPhase1<T>(ctx, "test.scan", FirstIn<T>{in}, n, seed, dTiles.get(), total, nDev);
        if (rc == MLSGPU_OK)
            rc = scanPhase2<T>(ctx, "test.scan", SecondIn<T>{in}, out, n, dTiles.get(), nDev);
    }
    hipStreamSynchronize(ctx->stream);
    return rc;
}

} // namespace

MLSGPU_API int mlsgpu_hip_test_scan(mlsgpu_ctx *ctx, uint32_t words, uint32_t form, const uint32_t *dIn, uint32_t *dPrefix,
                                    uint32_t *dValues, uint64_t n, const uint32_t seed[3], const uint32_t *dCount, uint32_t *dTotal)
{
    REQUIRE(ctx != nullptr && seed != nullptr && dTotal != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(words == 1 || words == 3, MLSGPU_ERR_INVALID);
    REQUIRE(form <= MLSGPU_TEST_SCAN_PHASES, MLSGPU_ERR_INVALID);
    REQUIRE(n == 0 || (dIn != nullptr && dPrefix != nullptr && dValues != nullptr), MLSGPU_ERR_INVALID);
    HIP_CHECK(hipSetDevice(ctx->device));
    return words == 1 ? testScan<uint32_t>(ctx, form, dIn, dPrefix, dValues, n, seed, dCount, dTotal)
                      : testScan<U3>(ctx, form, dIn, dPrefix, dValues, n, seed, dCount, dTotal);
}

/* ---- the batched sort ---- */

namespace
{

enum : uint32_t { SORT_GUARD_WORDS = 64, SORT_GUARD = 0xA55A5AA5u };

/* the temporaries of a lane, each with SORT_GUARD_WORDS words of SORT_GUARD behind its n elements */
template<typename K>
struct SortScratch
{
    DeviceArray<K> keys;
    DeviceArray<uint32_t> vals, hist;
    uint64_t n = 0;

    int alloc(mlsgpu_ctx *ctx, uint64_t count)
    {
        n = count;
        const uint32_t guardKeys = SORT_GUARD_WORDS * 4 / sizeof(K);
        PROPAGATE(keys.alloc(n + guardKeys));
        PROPAGATE(vals.alloc(n + SORT_GUARD_WORDS));
        PROPAGATE(hist.alloc(sortHistElems(n)));
        std::vector<uint32_t> guard(SORT_GUARD_WORDS, (uint32_t) SORT_GUARD);
        HIP_CHECK(hipMemcpyAsync(keys.get() + n, guard.data(), SORT_GUARD_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(vals.get() + n, guard.data(), SORT_GUARD_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));       /* `guard` leaves scope */
        return MLSGPU_OK;
    }

    int guardsIntact(uint32_t lane) const
    {
        uint32_t back[2][SORT_GUARD_WORDS];
        HIP_CHECK(hipMemcpy(back[0], keys.get() + n, SORT_GUARD_WORDS * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(back[1], vals.get() + n, SORT_GUARD_WORDS * 4, hipMemcpyDeviceToHost));
        for (uint32_t s = 0; s < 2; s++)
            for (uint32_t w = 0; w < SORT_GUARD_WORDS; w++)
                if (back[s][w] != SORT_GUARD)
                    return setError(MLSGPU_ERR_INVALID, "sort wrote behind lane %u's temporary %s (word %u)", lane,
                                    s == 0 ? "keys" : "values", w);
        return MLSGPU_OK;
    }
};

template<typename K>
int testSortBatch(mlsgpu_ctx *ctx, uint32_t count, void *const *dKeys, uint32_t *const *dValues, const uint64_t *n,
                  const uint32_t *const *dCount, uint32_t bits, bool iota, uint32_t doneBits, bool keysWanted, void *const *dKeysOut,
                  uint32_t *const *dValuesOut, uint32_t *side)
{
    SortScratch<K> scratch[MAX_LANES];
    SortJob<K> jobs[MAX_LANES];
    for (uint32_t k = 0; k < count; k++)
    {
        PROPAGATE(scratch[k].alloc(ctx, n[k]));
        jobs[k] = SortJob<K>{(K *) dKeys[k], dValues[k], scratch[k].keys.get(), scratch[k].vals.get(), n[k], scratch[k].hist.get(),
                             dCount != nullptr ? dCount[k] : (const uint32_t *) nullptr, SortResult<K>{nullptr, nullptr}};
    }
    int rc = radixSortBatch<K>(ctx, "test.sort", jobs, count, bits, iota, doneBits, keysWanted);
    for (uint32_t k = 0; k < count && rc == MLSGPU_OK; k++)
    {
        const SortResult<K> &res = jobs[k].result;
        const bool onA = res.keys == jobs[k].keysA && res.vals == jobs[k].valsA;
        const bool onB = res.keys == jobs[k].keysB && res.vals == jobs[k].valsB;
        if (!onA && !onB)
            rc = setError(MLSGPU_ERR_INVALID, "lane %u of the sort reports a result on neither side", k);
        else
        {
            side[k] = onA ? 0u : 1u;
            if (n[k] > 0 && keysWanted && dKeysOut != nullptr && dKeysOut[k] != nullptr)
                hipMemcpyAsync(dKeysOut[k], res.keys, n[k] * sizeof(K), hipMemcpyDeviceToDevice, ctx->stream);
            if (n[k] > 0 && dValuesOut != nullptr && dValuesOut[k] != nullptr)
                hipMemcpyAsync(dValuesOut[k], res.vals, n[k] * 4, hipMemcpyDeviceToDevice, ctx->stream);
        }
    }
    hipStreamSynchronize(ctx->stream);
    for (uint32_t k = 0; k < count && rc == MLSGPU_OK; k++)
        rc = scratch[k].guardsIntact(k);
    return rc;
}

} // namespace

MLSGPU_API int mlsgpu_hip_test_sort_batch(mlsgpu_ctx *ctx, uint32_t keyBytes, uint32_t count, void *const *dKeys, uint32_t *const *dValues,
                                          const uint64_t *n, const uint32_t *const *dCount, uint32_t bits, int iota, uint32_t doneBits,
                                          int keysWanted, void *const *dKeysOut, uint32_t *const *dValuesOut, uint32_t *side)
{
    REQUIRE(ctx != nullptr && dKeys != nullptr && dValues != nullptr && n != nullptr && side != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(keyBytes == 4 || keyBytes == 8, MLSGPU_ERR_INVALID);
    REQUIRE(count >= 1 && count <= MAX_LANES, MLSGPU_ERR_LENGTH);
    REQUIRE(bits <= keyBytes * 8 && doneBits <= bits, MLSGPU_ERR_INVALID);
    HIP_CHECK(hipSetDevice(ctx->device));
    return keyBytes == 4 ? testSortBatch<uint32_t>(ctx, count, dKeys, dValues, n, dCount, bits, iota != 0, doneBits, keysWanted != 0,
                                                   dKeysOut, dValuesOut, side)
                         : testSortBatch<uint64_t>(ctx, count, dKeys, dValues, n, dCount, bits, iota != 0, doneBits, keysWanted != 0,
                                                   dKeysOut, dValuesOut, side);
}
