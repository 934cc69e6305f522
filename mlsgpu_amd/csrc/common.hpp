/* Shared host/device plumbing of the HIP path: context, error reporting, launch timing, wave/block scans. */
#ifndef MLSGPU_AMD_COMMON_HPP
#define MLSGPU_AMD_COMMON_HPP

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mlsgpu_hip.h"

#define MLSGPU_API extern "C" __attribute__((visibility("default")))

namespace mlsgpu
{

/* ---------------------------------------------------------------- errors */

int setError(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_CHECK(expr)                                                                         \
    do {                                                                                        \
        hipError_t err__ = (expr);                                                              \
        if (err__ != hipSuccess)                                                                \
            return ::mlsgpu::setError(err__ == hipErrorOutOfMemory ? MLSGPU_ERR_NOMEM : MLSGPU_ERR_HIP, \
                                      "%s failed: %s (%s:%d)", #expr, hipGetErrorString(err__), \
                                      __FILE__, __LINE__);                                      \
    } while (0)

/* MLSGPU_ASSERT of src/errors.h:41-42: argument checks that raise length_error / invalid_argument */
#define REQUIRE(cond, code)                                                                     \
    do {                                                                                        \
        if (!(cond))                                                                            \
            return ::mlsgpu::setError(code, "requirement failed: %s (%s:%d)", #cond, __FILE__, __LINE__); \
    } while (0)

#define PROPAGATE(expr)                 \
    do {                                \
        int rc__ = (expr);              \
        if (rc__ != MLSGPU_OK)          \
            return rc__;                \
    } while (0)

/* Restores the calling thread's current device on every exit path.  Entry points that switch devices (peer appends, the
 * farm's dispatch to another GPU's copy stream) are called from worker threads in the middle of their own device's work;
 * anything device-implicit they do afterwards (event creation, hipMalloc) must still target their own GPU. */
struct DeviceGuard
{
    int saved = -1;
    DeviceGuard() { if (hipGetDevice(&saved) != hipSuccess) saved = -1; }
    ~DeviceGuard() { if (saved >= 0) (void) hipSetDevice(saved); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

/* Direct copies between two GPUs (xGMI) need peer access enabled in both directions; harmless when it already is, and
 * when the devices cannot reach each other the runtime stages the copy through the host. */
static inline void enablePeerAccess(int a, int b)
{
    if (a == b)
        return;
    DeviceGuard restore;
    for (int k = 0; k < 2; k++)
    {
        const int from = k ? b : a, to = k ? a : b;
        int can = 0;
        if (hipSetDevice(from) == hipSuccess && hipDeviceCanAccessPeer(&can, from, to) == hipSuccess && can)
            (void) hipDeviceEnablePeerAccess(to, 0);
        (void) hipGetLastError();       /* "already enabled" is not an error */
    }
}

/* ---------------------------------------------------------------- owned memory */

/*
 * Device memory that belongs to one object or one call: the pointer and the element capacity it was allocated with live
 * together, and the destructor frees.  The owner's device must be current.  alloc() and reserve() return the library's status
 * (and set its error text); a caller that can do without the buffer clears the sticky HIP error itself.
 */
template<typename T>
class DeviceArray
{
    T *p = nullptr;
    uint64_t cap = 0;

public:
    DeviceArray() = default;
    DeviceArray(DeviceArray &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DeviceArray &operator=(DeviceArray &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DeviceArray() { release(); }

    /* what alloc(n) takes from the device (never a zero-byte allocation) */
    static uint64_t bytes(uint64_t n) { return n ? n * sizeof(T) : 4; }
    /* exactly n elements, whatever was held before */
    int alloc(uint64_t n)
    {
        release();
        const hipError_t e = hipMalloc((void **) &p, bytes(n));
        if (e != hipSuccess)
        {
            p = nullptr;
            return setError(e == hipErrorOutOfMemory ? MLSGPU_ERR_NOMEM : MLSGPU_ERR_HIP, "cannot allocate %llu bytes of device memory: %s",
                            (unsigned long long) bytes(n), hipGetErrorString(e));
        }
        cap = n;
        return MLSGPU_OK;
    }
    /* at least n elements; grows only, and growing DISCARDS the contents.  A failure leaves the array empty, capacity 0 */
    int reserve(uint64_t n) { return p != nullptr && n <= cap ? MLSGPU_OK : alloc(n); }
    void release()
    {
        if (p) (void) hipFree(p);
        p = nullptr;
        cap = 0;
    }
    uint64_t capacity() const { return cap; }
    T *get() const { return p; }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};

/* The pinned-memory sibling, with a length n <= capacity: what a device -> host copy of n elements lands in */
template<typename T>
class PinnedArray
{
    T *p = nullptr;
    size_t n = 0, cap = 0;

public:
    PinnedArray() = default;
    PinnedArray(const PinnedArray &) = delete;
    PinnedArray &operator=(const PinnedArray &) = delete;
    ~PinnedArray() { release(); }

    /* exactly `count` elements (hipHostMalloc's flags), whatever was held before; a failure leaves the array empty */
    int alloc(size_t count, unsigned int flags = hipHostMallocDefault)
    {
        release();
        if (hipHostMalloc((void **) &p, count * sizeof(T), flags) != hipSuccess)
        {
            p = nullptr;
            return setError(MLSGPU_ERR_NOMEM, "cannot allocate %zu bytes of pinned memory", count * sizeof(T));
        }
        n = cap = count;
        return MLSGPU_OK;
    }
    /* `count` elements, contents undefined: grows with a quarter of headroom, never shrinks */
    int resize(size_t count, unsigned int flags = hipHostMallocDefault)
    {
        if (count > cap)
            PROPAGATE(alloc(count + count / 4 + 1024, flags));
        n = count;
        return MLSGPU_OK;
    }
    void release()
    {
        if (p) (void) hipHostFree(p);
        p = nullptr;
        n = cap = 0;
    }
    void clear() { n = 0; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    T *data() const { return p; }
    const T *begin() const { return p; }
    const T *end() const { return p + n; }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};

/* ---------------------------------------------------------------- context */

struct Stat
{
    double totalMs = 0.0;
    uint64_t launches = 0;
};

struct PendingTiming
{
    int nameId;
    hipEvent_t start, stop;
};

} // namespace mlsgpu

struct mlsgpu_ctx
{
    int device = 0;
    uint64_t serial = 0;              /* unique per context: call sites cache stat ids against it, not the address */
    hipStream_t stream = nullptr;
    bool ownStream = false;
    bool timing = false;
    std::vector<std::string> statNames;
    std::map<std::string, int> statIds;
    std::vector<mlsgpu::Stat> stats;
    std::vector<mlsgpu::PendingTiming> pending;
    std::vector<hipEvent_t> eventPool;
    /* device scratch that entry points without an object of their own (mlsgpu_hip_bucket) keep between calls;
     * released with the context */
    std::map<std::string, std::shared_ptr<void> > scratchCache;

    /* one-launch scans (primitives.hpp): a flag word per (lane, tile), never cleared -- a launch's flags carry its epoch */
    uint32_t *dScanFlags = nullptr;
    uint32_t scanEpoch = 0;
    uint32_t scanTicketBase[MLSGPU_MAX_BATCH] = {};     /* what lane k's ticket counter reads when the next launch begins */
    /* flags + epoch of the next one-launch scan, the lanes' ticket counters and what they read now; a launch of `gridX`
     * workgroups for each of `count` lanes is accounted for */
    int scanFlags(uint32_t **flags, uint32_t *epoch, uint32_t **tickets, uint32_t *bases, uint32_t gridX, uint32_t count);

    int statId(const char *name);
    /* a sample of one of the reference's non-timer statistics (Statistics::Counter / Variable: marching.overflow,
     * marching.slices.nonempty, marching.shipouts; src/marching.cpp:350-352): the sum in the "ms" column, the samples in the
     * launch column of mlsgpu_hip_ctx_get_stat / _dump_stats */
    void addValue(const char *name, double value)
    {
        mlsgpu::Stat &st = stats[(size_t) statId(name)];
        st.totalMs += value;
        st.launches += 1;
    }
    int beginTiming(int id);          /* returns index into pending or -1 */
    void endTiming(int pendingIdx);
    int resolveTimings();             /* synchronises the stream */
};

namespace mlsgpu
{

/*
 * Small device -> host read-backs on the critical path (the octree's entry count, Marching's swathe totals and welded
 * counts: 4 to 24 bytes each, three per bucket, each followed by a host decision).  A hipMemcpyAsync of a few bytes plus
 * hipStreamSynchronize costs a copy-engine submission and a signal wait; here a one-thread kernel stores the words straight
 * into mapped, coherent pinned memory, a sequence number behind a system-scope fence, and the host polls that word.  The
 * stream is not drained: what the host enqueues next lands behind the kernel that published.
 */
struct HostMailbox
{
    enum { WORDS = 64 };            /* six words per bucket of a batch (MAX_LANES buckets) and room to spare */
    uint32_t *host = nullptr;       /* [0] = sequence number of the last publication, [1 .. WORDS] = payload */
    uint32_t *dev = nullptr;        /* the same memory as the device sees it */
    uint32_t seq = 0;

    int create();
    void destroy();
    /* for a kernel that publishes by itself (payload words first, then a system-scope fence, then the sequence number into
     * dev[0]): the sequence number it has to write; wait() then waits for that one */
    uint32_t reserve()
    {
        seq++;
        if (seq == 0)
            seq = 1;
        return seq;
    }
    /* enqueue: copy `words` 32-bit words from device memory `src` to the mailbox (on `stream`) */
    int publish(hipStream_t stream, const void *src, uint32_t words);
    /* the same for a batch: `wordsEach` words from each of `count` device addresses, laid out one source after the other */
    int publishGather(hipStream_t stream, const void *const *srcs, uint32_t count, uint32_t wordsEach);
    /* block until the last publication has landed; the payload is host[1 ..] */
    int wait(hipStream_t stream);
    const uint32_t *payload() const { return host + 1; }
};

/* Launch a kernel on the context's stream, timing it under a reference stat name when enabled. */
#define LAUNCH(ctx, statName, kernel, grid, block, ...) LAUNCH_LDS(ctx, statName, kernel, grid, block, 0, __VA_ARGS__)

/* the same with `ldsBytes` of dynamic LDS on top of the kernel's static allocation */
#define LAUNCH_LDS(ctx, statName, kernel, grid, block, ldsBytes, ...)                         \
    do {                                                                                      \
        static thread_local int statId__ = -1;                                                \
        static thread_local uint64_t statCtx__ = 0;                                           \
        int pend__ = -1;                                                                      \
        if ((ctx)->timing) {                                                                  \
            if (statCtx__ != (ctx)->serial) { statId__ = (ctx)->statId(statName); statCtx__ = (ctx)->serial; } \
            pend__ = (ctx)->beginTiming(statId__);                                            \
        }                                                                                     \
        hipLaunchKernelGGL(kernel, grid, block, ldsBytes, (ctx)->stream, __VA_ARGS__);        \
        if (pend__ >= 0) (ctx)->endTiming(pend__);                                            \
        HIP_CHECK(hipGetLastError());                                                         \
    } while (0)

/*
 * Batches.  A device worker may take several buckets (the SubItems of a WorkItem, src/workers.h:148-181) through the path
 * in lock-step: every kernel has a bucket dimension -- blockIdx.y selects the LANE, whose arguments are one element of an
 * array passed by value in the kernel-argument segment (read through the scalar cache, no upload of a parameter block),
 * grid.x covers the largest lane and the workgroups beyond a smaller lane's own extent leave at once.  A single bucket is a
 * batch of one: same kernels, same results.
 * A kernel COPIES its lane's element (`const Args A = lanes.a[blockIdx.y];`): the fields then live in scalar registers as
 * those of a by-value parameter do.  Through a reference the compiler re-loads a field wherever it is used under a condition
 * -- latticeMask, bound by scalar / vector issue, ran 18 % slower with ~100 kernel-argument loads in its loop.
 * The host fills the array with packLanes(count, make) and nothing else does: the slots at or beyond the live count are
 * value-initialised and never read.  A launch's grid.y -- or the lane count of a kernel that loops over the lanes -- MUST be
 * the count its lanes were packed with.
 */
enum { MAX_LANES = MLSGPU_MAX_BATCH };
template<typename A>
struct Lanes
{
    A a[MAX_LANES];
};

/* a[k] = make(k) for the live lanes k < count (<= MAX_LANES: the callers' REQUIREs) */
template<typename A, typename Make>
static inline Lanes<A> packLanes(uint32_t count, Make make)
{
    Lanes<A> lanes{};
    for (uint32_t k = 0; k < count; k++)
        lanes.a[k] = make(k);
    return lanes;
}

/* the largest extent(k) over the live lanes: a launch's grid.x */
template<typename Extent>
static inline uint32_t mostOfLanes(uint32_t count, Extent extent)
{
    uint32_t most = 0;
    for (uint32_t k = 0; k < count; k++)
        most = extent(k) > most ? extent(k) : most;
    return most;
}

static inline uint32_t divUp(uint64_t a, uint64_t b) { return (uint32_t) ((a + b - 1) / b); }
static inline uint32_t roundUp(uint32_t a, uint32_t b) { return (a + b - 1) / b * b; }

/* fill.hip, for the sink's hole filling (mesher.hip): dPinned[g] = 1 for each of the n packed xyz rows that equals, bit for
 * bit, a row of another chunk, 0 for the others; chunk c holds the rows [starts[c], starts[c + 1]) (host memory).  Blocks. */
int seamMask(mlsgpu_ctx *ctx, const float *dVertices, uint64_t n, const uint64_t *starts, uint32_t numChunks, uint8_t *dPinned);

/* compact.hip, for the sink's compact read-back (mesher.hip): mlsgpu_hip_mesh_compact with the blob going to dOut (device
 * memory) or, through device scratch of the blob's size, to hostOut (host memory, pinned or not); the one that is given holds
 * `capacity` bytes.  Blocks. */
int compactMesh(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles, uint64_t numTriangles,
                uint32_t vertexBits, void *dOut, void *hostOut, uint64_t capacity, mlsgpu_compact_stats *stats);

/* ---------------------------------------------------------------- device helpers */

#ifdef __HIPCC__

#define WAVE 64

__device__ __forceinline__ uint32_t laneId()
{
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

/* number of set bits of `mask` strictly below this lane */
__device__ __forceinline__ uint32_t popcBelow(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
}

/* Cross-lane steps as DPP modifiers of the vector instruction itself (gfx9: row_shr, row_bcast15 / 31, wave_shr) instead
 * of ds_bpermute round trips through the LDS crossbar: a scan is six dependent VALU instructions, not six LDS latencies.
 * update_dpp(old, src, ctrl, row_mask, bank_mask, bound_ctrl = false): lanes without a source lane, or outside the masks,
 * get `old`. */
#define DPP_ROW_SHR(n) (0x110 + (n))
#define DPP_WAVE_SHR1 0x138
#define DPP_ROW_BCAST15 0x142
#define DPP_ROW_BCAST31 0x143

/* inclusive prefix sum across the 64 lanes of a wave */
__device__ __forceinline__ uint32_t waveInclusiveScan(uint32_t v)
{
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_SHR(1), 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_SHR(2), 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_SHR(4), 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_SHR(8), 0xf, 0xf, false);
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_BCAST15, 0xa, 0xf, false);   /* rows 1, 3 += row 0 / 2 */
    v += (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_BCAST31, 0xc, 0xf, false);   /* rows 2, 3 += rows 0 + 1 */
    return v;
}

/* The reductions below read lane 63 of the scan, and the shifts use the gfx9 wave_shr / wave_shl DPP controls: they need a
 * FULL, CONVERGENT wave64 (every caller in this library is one; an inactive lane 63 would hand back stale register
 * contents, where a ds_bpermute version reads zero from inactive lanes). */
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "the wave helpers are written for gfx950 (wave64, gfx9 DPP controls)"
#endif

/* the sum over the wave, in every lane */
__device__ __forceinline__ uint32_t waveSum(uint32_t v)
{
    return (uint32_t) __builtin_amdgcn_readlane((int) waveInclusiveScan(v), 63);
}

/* maximum over the wave, in every lane (wave-uniform) */
__device__ __forceinline__ uint32_t waveMax(uint32_t v)
{
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_SHR(1), 0xf, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_SHR(2), 0xf, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_SHR(4), 0xf, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_SHR(8), 0xf, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_BCAST15, 0xa, 0xf, false));
    v = max(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_ROW_BCAST31, 0xc, 0xf, false));
    return (uint32_t) __builtin_amdgcn_readlane((int) v, 63);
}

/* value of lane - 1; lane 0 gets zero */
__device__ __forceinline__ uint32_t waveShiftUp1(uint32_t v)
{
    return (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, DPP_WAVE_SHR1, 0xf, 0xf, false);
}

/* value of lane + 1; lane 63 gets zero */
__device__ __forceinline__ uint32_t waveShiftDown1(uint32_t v)
{
    return (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

__device__ __forceinline__ uint32_t readLane(uint32_t v, int lane)
{
    return __builtin_amdgcn_readlane(v, lane);
}

#endif /* __HIPCC__ */

} // namespace mlsgpu

#endif
