/*
 * Hole filling of an indexed triangle mesh that is resident in HBM: every small boundary loop gets a fan of triangles to the
 * mean of its vertices.  The reference has no counterpart.  The contract (include/mlsgpu_hip.h, DESIGN.md "Hole filling") is
 * written so that every output is an integer sum or one correctly rounded operation away from one: the result depends
 * neither on the schedule nor on how the triangles are ordered.
 *
 *   extent     over the coordinates: the largest |coordinate| (its bits), the coordinates that are not finite
 *   classify   a thread per triangle: its class, and its three directed sides as keys from << b | to
 *   sort       the keys: equal sides become one run, and the opposite side of a -> b is found by a binary search for b -> a
 *   sides      over the records: a BOUNDARY side is alone in its run and has no opposite.  It counts at both its ends,
 *              unites them in the boundary forest (unionfind.hpp) and stores next[from] = to
 *   loops      a thread per boundary vertex: its root -- the smallest vertex of its component, whatever the schedule -- gets
 *              the component's length and its irregular / pinned flags
 *   sums       over the boundary vertices: the counts of the contract's steps 4 and 5 (at the roots), and the three
 *              fixed-point sums of the loops that will be filled                                         -- one read-back --
 *   number     a scan over the vertices with the flag at the roots of the filled loops: loop j, and its new vertex V + j
 *   emit       a scan over the vertices with the flag at the vertices of the filled loops: vertex a writes (next[a], a, V + j)
 *
 * No kernel walks a loop: no running time depends on a loop's length (meshpost.hpp's forEachRoot combines the lanes of a wave
 * that share a root).  An index >= V is compared and counted, never used as an address; no address depends on a coordinate.
 *
 * Scratch belongs to the call: 72 bytes per triangle (three records: the two sides of the sort's 64-bit keys and 32-bit
 * values), 52 bytes per vertex (parent, out- and in-count, next, length, flags, loop number 4 each, the sums 24), the sort's
 * histogram (4 KB per 4096 records) and the scan's tile sums.
 */
#include "meshpost.hpp"
#include "unionfind.hpp"

#include <cmath>

using namespace mlsgpu;

namespace
{

enum
{
    C_OUT_OF_RANGE = 0,
    C_DEGENERATE = 1,
    C_BOUNDARY_EDGES = 2,
    C_IRREGULAR_EDGES = 3,
    C_LOOPS = 4,
    C_FILLED_LOOPS = 5,
    C_LONG_LOOPS = 6,
    C_PINNED_LOOPS = 7,
    C_FILLED_EDGES = 8,
    C_LONGEST_LOOP = 9,
    C_NON_FINITE = 10,          /* input coordinates */
    C_INPUT_MAX = 11,           /* the bits of the largest |coordinate| */
    C_FAILED = 12,              /* the union-find's retry bound was reached (its low 32 bits are the flag) */
    C_WORDS = 13
};

enum
{
    F_IRREGULAR = 1,            /* a vertex of the component has not exactly one side out and one in */
    F_PINNED = 2                /* a vertex of the component is pinned */
};

/* LOOP_BLOCKS for the sides kernel, which waits for its binary searches: more waves in flight */
const uint32_t SIDES_BLOCKS = 4096;

/* step 5 of the contract, from what the loops kernel left at a component's root */
__device__ __forceinline__ bool isLoop(uint32_t length, uint32_t flags) { return length != 0 && (flags & F_IRREGULAR) == 0; }
__device__ __forceinline__ bool isFilled(uint32_t length, uint32_t flags, uint32_t maxEdges)
{
    return isLoop(length, flags) && length <= maxEdges && (flags & F_PINNED) == 0;
}

/* A workgroup loops over the 3 V coordinates and sends its maximum and its count once. */
__global__ __launch_bounds__(256) void extentKernel(const float *vertices, uint64_t numCoordinates, Counter *counters)
{
    __shared__ GroupCounts<1, 1> totals;
    totals.clear();
    const int at[2] = {C_NON_FINITE, C_INPUT_MAX};
    uint32_t most = 0, bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < numCoordinates; i += (uint64_t) gridDim.x * blockDim.x)
    {
        const float x = vertices[i];
        most = max(most, __float_as_uint(fabsf(x)));
        bad += isfinite(x) ? 0u : 1u;
    }
    totals.add(0, bad);
    totals.raise(0, most);
    totals.flush(counters, at);
}

__global__ __launch_bounds__(256) void identityKernel(uint32_t *parent, uint64_t numVertices)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v < numVertices)
        parent[v] = (uint32_t) v;
}

/* Step 1: the three directed sides of a triangle; three dead records for one that takes no part */
__global__ __launch_bounds__(256) void classifyKernel(const uint32_t *tri, uint64_t numTriangles, SideKeys K, uint64_t *keys,
                                                      Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    const TriangleDefect d = defectOf(i, K.numVertices);
    tally(d.outOfRange, &counters[C_OUT_OF_RANGE]);
    tally(d.degenerate, &counters[C_DEGENERATE]);
#pragma unroll
    for (int k = 0; k < 3; k++)
        keys[3 * t + k] = d.none() ? K.keyOf(i[k], i[k == 2 ? 0 : k + 1]) : K.dead();
}

/* Steps 2 and 3.  A vertex with several sides out keeps whichever `next` was stored last: it is irregular, and the next of an
 * irregular vertex is never read.  A workgroup loops over the records (at most 2^32 / SIDES_BLOCKS of them: its count fits 32
 * bits) and sends its count once: a real chunk has a boundary side in most waves. */
__global__ __launch_bounds__(256) void sidesKernel(Records R, uint32_t *outCount, uint32_t *inCount, uint32_t *next, uint32_t *parent,
                                                   Counter *counters)
{
    __shared__ GroupCounts<1> sides;
    sides.clear();
    const int at[1] = {C_BOUNDARY_EDGES};
    uint32_t count = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < R.n; i += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t key = R.keys[i], from = R.fromOf(key);
        if (from >= R.numVertices)
            continue;           /* the record of a triangle that takes no part */
        const uint32_t to = R.toOf(key);
        if (!R.single(i, key) || R.has(R.keyOf(to, from)))
            continue;
        count++;
        atomicAdd(&outCount[from], 1u);
        atomicAdd(&inCount[to], 1u);
        next[from] = to;
        unite(parent, (uint32_t) from, to, reinterpret_cast<uint32_t *>(&counters[C_FAILED]), UNION_SHORTCUT);
    }
    sides.add(0, count);
    sides.flush(counters, at);
}

/* Step 4, first half.  The forest is finished (a launch lies between): a root is its component's smallest vertex.  Every
 * boundary vertex is re-parented to its root, for the kernels behind this one; a walk of another thread that passes through
 * it meanwhile meets the old parent or the root, both its ancestors.  The lanes of the wave that share a root send ONE add
 * and at most one or.  Every lane stays to the end. */
__global__ __launch_bounds__(256) void loopsKernel(uint64_t numVertices, const uint32_t *outCount, const uint32_t *inCount,
                                                   const uint8_t *pinned, uint32_t *parent, uint32_t *length, uint32_t *flags)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t out = 0, in = 0;
    if (v < numVertices)
    {
        out = outCount[v];
        in = inCount[v];
    }
    const bool on = (out | in) != 0;
    uint32_t root = 0;
    bool irregular = false, pin = false;
    if (on)
    {
        root = findRoot(parent, (uint32_t) v);
        __hip_atomic_store(&parent[v], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        irregular = out != 1 || in != 1;
        pin = pinned != nullptr && pinned[v] != 0;
    }
    forEachRoot(on, root, [&](uint32_t r, bool same, uint64_t sharers, bool leads) {
        const uint32_t bits = (__ballot(same && irregular) != 0 ? F_IRREGULAR : 0) | (__ballot(same && pin) != 0 ? F_PINNED : 0);
        if (leads)
        {
            atomicAdd(&length[r], (uint32_t) __popcll(sharers));
            if (bits != 0)
                atomicOr(&flags[r], bits);
        }
    });
}

/* Steps 4 and 5, and the sums of step 7 (Q is meshpost.hpp's quantise: a finite input stays within 2^31, and a call with
 * another is refused by its count of them).  parent[] holds roots now, length[] and flags[] are complete.  A root counts its
 * component; a vertex of an irregular component counts its sides out; a vertex of a loop that will be filled adds its
 * quantised position to the root's sums, the lanes of the wave that share the root through ONE lane.  A workgroup loops over
 * blocks of 256 vertices -- every lane of it as often, so that the wave is whole where its lanes talk -- and sends its seven
 * counts and its maximum once: a real chunk has tens of thousands of small loops (its counts fit 32 bits: filledEdges and
 * irregularEdges are at most 3 T < 2^32 over the whole launch). */
__global__ __launch_bounds__(256) void sumsKernel(const float *vertices, uint64_t numVertices, const uint32_t *outCount, const uint32_t *inCount,
                                                  const uint32_t *parent, const uint32_t *length, const uint32_t *flags, uint32_t maxEdges,
                                                  Counter *sums, Counter *counters)
{
    enum { LOOPS, FILLED, LONG, PINNED, FILLED_EDGES, IRREGULAR_EDGES, COUNTS };
    const int at[COUNTS + 1] = {C_LOOPS, C_FILLED_LOOPS, C_LONG_LOOPS, C_PINNED_LOOPS, C_FILLED_EDGES, C_IRREGULAR_EDGES, C_LONGEST_LOOP};
    __shared__ GroupCounts<COUNTS, 1> totals;
    totals.clear();
    const double scale = powerOfTwo(30 - exponentOfBits((uint32_t) counters[C_INPUT_MAX]));
    uint32_t count[COUNTS] = {0, 0, 0, 0, 0, 0}, longest = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < numVertices; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t v = base + threadIdx.x;
        uint32_t out = 0, in = 0;
        if (v < numVertices)
        {
            out = outCount[v];
            in = inCount[v];
        }
        const bool on = (out | in) != 0;
        uint32_t root = 0, n = 0, f = 0;
        if (on)
        {
            root = parent[v];
            n = length[root];
            f = flags[root];
        }
        const bool loop = on && root == (uint32_t) v && isLoop(n, f);
        const bool isLong = loop && n > maxEdges;
        const bool isPinned = loop && !isLong && (f & F_PINNED) != 0;
        const bool filled = loop && !isLong && !isPinned;
        count[LOOPS] += loop ? 1u : 0u;
        count[FILLED] += filled ? 1u : 0u;
        count[LONG] += isLong ? 1u : 0u;
        count[PINNED] += isPinned ? 1u : 0u;
        count[FILLED_EDGES] += filled ? n : 0u;
        count[IRREGULAR_EDGES] += on && (f & F_IRREGULAR) != 0 ? out : 0u;
        longest = max(longest, loop ? n : 0u);

        const bool adds = on && isFilled(n, f, maxEdges);
        long long q[3] = {0, 0, 0};
        if (adds)
#pragma unroll
            for (int k = 0; k < 3; k++)
                q[k] = quantise(vertices[3 * v + k], scale);
        forEachRoot(adds, root, [&](uint32_t r, bool same, uint64_t, bool leads) {
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                const long long s = waveSum64(same ? q[k] : 0);
                if (leads)
                    atomicAdd(&sums[3 * (uint64_t) r + k], (Counter) s);
            }
        });
    }
#pragma unroll
    for (int k = 0; k < COUNTS; k++)
        totals.add(k, count[k]);
    totals.raise(0, longest);
    totals.flush(counters, at);
}

/* Step 8: the flag stands at the root -- the smallest vertex -- of every filled loop.  (length is non-zero at roots only.) */
struct FilledRootIn
{
    const uint32_t *length, *flags;
    uint32_t maxEdges;
    __device__ __forceinline__ uint32_t operator()(uint64_t v) const { return isFilled(length[v], flags[v], maxEdges) ? 1u : 0u; }
};
/* ... and the root writes the loop's number and its new vertex, step 7 */
struct NewVertexOut
{
    const uint32_t *length;
    const Counter *sums;
    uint32_t *loopOf;
    float *outVertices;         /* behind the input's */
    double invScale;
    __device__ __forceinline__ void operator()(uint64_t v, uint32_t before, uint32_t flag) const
    {
        if (!flag)
            return;
        loopOf[v] = before;
        const double n = (double) length[v];
#pragma unroll
        for (int k = 0; k < 3; k++)
            outVertices[3 * (uint64_t) before + k] = (float) (((double) (long long) sums[3 * v + k] / n) * invScale);
    }
};

/* Steps 9 and 10: the flag stands at every vertex of a filled loop (each has exactly one side out) */
struct FilledVertexIn
{
    const uint32_t *outCount, *parent, *length, *flags;
    uint32_t maxEdges;
    __device__ __forceinline__ uint32_t operator()(uint64_t v) const
    {
        if (outCount[v] == 0)
            return 0u;
        const uint32_t r = parent[v];
        return isFilled(length[r], flags[r], maxEdges) ? 1u : 0u;
    }
};
struct NewTriangleOut
{
    const uint32_t *parent, *next, *loopOf;
    uint32_t *outTriangles;     /* behind the input's */
    uint32_t firstNew;          /* V */
    __device__ __forceinline__ void operator()(uint64_t v, uint32_t before, uint32_t flag) const
    {
        if (!flag)
            return;
        outTriangles[3 * (uint64_t) before] = next[v];
        outTriangles[3 * (uint64_t) before + 1] = (uint32_t) v;
        outTriangles[3 * (uint64_t) before + 2] = firstNew + loopOf[parent[v]];
    }
};

/* ---- the seams of a sink's chunks (mlsgpu::seamMask) ---- */

__global__ __launch_bounds__(256) void zKeysKernel(const float *vertices, uint64_t n, uint32_t *keys)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        keys[i] = __float_as_uint(vertices[3 * i + 2]);
}

__global__ __launch_bounds__(256) void xyKeysKernel(const float *vertices, const uint32_t *order, uint64_t n, uint64_t *keys)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t v = order[i];
    keys[i] = (uint64_t) __float_as_uint(vertices[3 * v]) << 32 | __float_as_uint(vertices[3 * v + 1]);
}

/* the rows in sorted order: equal rows are neighbours, and within them the vertex numbers -- hence the chunks -- rise */
struct Rows
{
    const float *vertices;
    const uint32_t *order;
    uint64_t n;
    __device__ __forceinline__ bool head(uint64_t i) const
    {
        if (i == 0)
            return true;
        const uint64_t a = order[i - 1], b = order[i];
#pragma unroll
        for (int k = 0; k < 3; k++)
            if (__float_as_uint(vertices[3 * a + k]) != __float_as_uint(vertices[3 * b + k]))
                return true;
        return false;
    }
};
struct RunHeadIn
{
    Rows R;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return R.head(i) ? 1u : 0u; }
};
/* runOf[i] = the run of row i; runFirst[run] = its first row */
struct RunOut
{
    uint32_t *runOf, *runFirst;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t before, uint32_t head) const
    {
        runOf[i] = before + head - 1;
        if (head)
            runFirst[before] = (uint32_t) i;
    }
};

/* the chunk that global vertex g lies in: the last one that starts at or before it (empty chunks start where the next does) */
__device__ __forceinline__ uint32_t chunkOfVertex(const uint64_t *starts, uint32_t numChunks, uint64_t g)
{
    uint32_t lo = 0, hi = numChunks;
    while (hi - lo > 1)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (starts[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

/* a row is pinned if its run reaches into another chunk: the chunks rise along a run, so its ends tell */
__global__ __launch_bounds__(256) void markSeamsKernel(Rows R, const uint32_t *runOf, const uint32_t *runFirst, const uint32_t *numRuns,
                                                       const uint64_t *starts, uint32_t numChunks, uint8_t *pinned)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n)
        return;
    const uint32_t run = runOf[i];
    const uint64_t first = runFirst[run], last = (run + 1 < *numRuns ? (uint64_t) runFirst[run + 1] : R.n) - 1;
    const uint64_t g = R.order[i];
    uint8_t pin = 0;
    if (first != last)
    {
        const uint32_t mine = chunkOfVertex(starts, numChunks, g);
        pin = chunkOfVertex(starts, numChunks, R.order[first]) != mine || chunkOfVertex(starts, numChunks, R.order[last]) != mine;
    }
    pinned[g] = pin;
}

} // namespace

/* pinned[g] = 1 for every one of the n vertices whose 12 bytes equal those of a vertex of another chunk; chunk c holds the
 * vertices [starts[c], starts[c + 1]).  A stable sort by z and then by (x, y) with the vertex number as the value brings equal
 * rows together; one scan numbers the runs.  Scratch: 40 bytes per vertex and the sort's histogram, freed on return. */
int mlsgpu::seamMask(mlsgpu_ctx *ctx, const float *dVertices, uint64_t n, const uint64_t *starts, uint32_t numChunks, uint8_t *dPinned)
{
    REQUIRE(n < (uint64_t(1) << 32) && numChunks >= 1, MLSGPU_ERR_LENGTH);
    if (n == 0)
        return MLSGPU_OK;
    const dim3 B(256), G(divUp(n, 256));
    DeviceArray<uint32_t> zA, zB, valsA, valsB, hist, tileSums, numRuns;
    DeviceArray<uint64_t> xyA, xyB, dStarts;
    PROPAGATE(zA.alloc(n));
    PROPAGATE(zB.alloc(n));
    PROPAGATE(valsA.alloc(n));
    PROPAGATE(valsB.alloc(n));
    PROPAGATE(xyA.alloc(n));
    PROPAGATE(xyB.alloc(n));
    PROPAGATE(hist.alloc(sortHistElems(n)));
    PROPAGATE(tileSums.alloc((uint64_t) scanTiles(n) + 1));
    PROPAGATE(numRuns.alloc(1));
    PROPAGATE(dStarts.alloc(numChunks + 1));
    HIP_CHECK(hipMemcpyAsync(dStarts.get(), starts, (numChunks + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, "kernel.fill.seams", zKeysKernel, G, B, dVertices, n, zA.get());
    SortResult<uint32_t> byZ = {nullptr, nullptr};
    PROPAGATE(radixSort<uint32_t>(ctx, "kernel.fill.seams", zA, valsA, zB, valsB, n, 32, true, hist, nullptr, &byZ, nullptr, 0, false));
    uint32_t *const other = byZ.vals == valsA.get() ? valsB.get() : valsA.get();
    LAUNCH(ctx, "kernel.fill.seams", xyKeysKernel, G, B, dVertices, (const uint32_t *) byZ.vals, n, xyA.get());
    SortResult<uint64_t> sorted = {nullptr, nullptr};
    PROPAGATE(radixSort<uint64_t>(ctx, "kernel.fill.seams", xyA, byZ.vals, xyB, other, n, 64, false, hist, nullptr, &sorted, nullptr, 0, false));
    /* the z keys are free again: the run of every row and the first row of every run */
    const Rows R = {dVertices, sorted.vals, n};
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.fill.seams", RunHeadIn{R}, RunOut{zA.get(), zB.get()}, n, 0u, tileSums.get(), numRuns.get())));
    LAUNCH(ctx, "kernel.fill.seams", markSeamsKernel, G, B, R, (const uint32_t *) zA.get(), (const uint32_t *) zB.get(),
           (const uint32_t *) numRuns.get(), (const uint64_t *) dStarts.get(), numChunks, dPinned);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));       /* the scratch goes with the call */
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesh_fill_holes(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                          uint64_t numTriangles, uint32_t maxEdges, const uint8_t *dPinned, float *dOutVertices,
                                          uint64_t capVertices, uint32_t *dOutTriangles, uint64_t capTriangles, mlsgpu_fill_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(maxEdges >= 3 && maxEdges <= MLSGPU_FILL_MAX_EDGES, MLSGPU_ERR_INVALID);
    /* the sort's values and tile counts are 32-bit, and so are the indices of a triangle */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || dVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->numVertices = numVertices;
    stats->numTriangles = numTriangles;

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t nv = numVertices, nt = numTriangles, n = 3 * nt;
    const SideKeys K = SideKeys::of(nv);
    const dim3 B(256);
    DeviceArray<Counter> counters, sums;
    DeviceArray<uint32_t> parent, outCount, inCount, next, length, flags, loopOf, tileSums;
    SortScratch records;
    Counter h[C_WORDS];
    std::memset(h, 0, sizeof(h));
    const bool sides = nv > 0 && nt > 0;        /* without vertices every triangle is out of range */
    if (nv > 0)
    {
        const uint64_t tileElems = (uint64_t) scanTiles(nv) + 1;
        PROPAGATE(counters.alloc(C_WORDS));
        PROPAGATE(sums.alloc(3 * nv));
        PROPAGATE(parent.alloc(nv));
        PROPAGATE(outCount.alloc(nv));
        PROPAGATE(inCount.alloc(nv));
        PROPAGATE(next.alloc(nv));
        PROPAGATE(length.alloc(nv));
        PROPAGATE(flags.alloc(nv));
        PROPAGATE(loopOf.alloc(nv));
        PROPAGATE(tileSums.alloc(tileElems));
        double scratch = (double) (counters.bytes(C_WORDS) + sums.bytes(3 * nv) + 7 * parent.bytes(nv) + tileSums.bytes(tileElems));
        if (sides)
        {
            PROPAGATE(records.alloc(n));
            scratch += (double) records.bytes();
        }
        if (ctx->timing)
            ctx->addValue("fill.scratch.bytes", scratch);

        HIP_CHECK(hipMemsetAsync(counters.get(), 0, C_WORDS * sizeof(Counter), ctx->stream));
        HIP_CHECK(hipMemsetAsync(sums.get(), 0, 3 * nv * sizeof(Counter), ctx->stream));
        HIP_CHECK(hipMemsetAsync(outCount.get(), 0, nv * sizeof(uint32_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(inCount.get(), 0, nv * sizeof(uint32_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(length.get(), 0, nv * sizeof(uint32_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(flags.get(), 0, nv * sizeof(uint32_t), ctx->stream));
        LAUNCH(ctx, "kernel.fill.extent", extentKernel, dim3(std::min(divUp(3 * nv, 256), LOOP_BLOCKS)), B, dVertices, 3 * nv, counters.get());
        if (sides)
        {
            LAUNCH(ctx, "kernel.fill.init", identityKernel, dim3(divUp(nv, 256)), B, parent.get(), nv);
            LAUNCH(ctx, "kernel.fill.classify", classifyKernel, dim3(divUp(nt, 256)), B, dTriangles, nt, K, records.keys(), counters.get());
            Records R;
            PROPAGATE(records.sort(ctx, "kernel.fill.sort", K, true, &R));
            LAUNCH(ctx, "kernel.fill.sides", sidesKernel, dim3(std::min(divUp(n, 256), SIDES_BLOCKS)), B, R, outCount.get(), inCount.get(), next.get(), parent.get(),
                   counters.get());
            LAUNCH(ctx, "kernel.fill.loops", loopsKernel, dim3(divUp(nv, 256)), B, nv, (const uint32_t *) outCount.get(),
                   (const uint32_t *) inCount.get(), dPinned, parent.get(), length.get(), flags.get());
            LAUNCH(ctx, "kernel.fill.sums", sumsKernel, dim3(std::min(divUp(nv, 256), LOOP_BLOCKS)), B, dVertices, nv, (const uint32_t *) outCount.get(),
                   (const uint32_t *) inCount.get(), (const uint32_t *) parent.get(), (const uint32_t *) length.get(),
                   (const uint32_t *) flags.get(), maxEdges, sums.get(), counters.get());
        }
        HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    else
        h[C_OUT_OF_RANGE] = nt;         /* every index is >= 0 vertices */
    if (h[C_NON_FINITE] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh fill holes: %llu coordinates are not finite", h[C_NON_FINITE]);
    if ((uint32_t) h[C_FAILED] != 0)
        return setError(MLSGPU_ERR_HIP, "mesh fill holes: the union-find did not settle within its retry bound");

    const int e = exponentOfBits((uint32_t) h[C_INPUT_MAX]);
    stats->outOfRangeTriangles = h[C_OUT_OF_RANGE];
    stats->degenerateTriangles = h[C_DEGENERATE];
    stats->boundaryEdges = h[C_BOUNDARY_EDGES];
    stats->irregularEdges = h[C_IRREGULAR_EDGES];
    stats->loops = h[C_LOOPS];
    stats->filledLoops = h[C_FILLED_LOOPS];
    stats->longLoops = h[C_LONG_LOOPS];
    stats->pinnedLoops = h[C_PINNED_LOOPS];
    stats->filledEdges = h[C_FILLED_EDGES];
    stats->longestLoop = h[C_LONGEST_LOOP];
    stats->outVertices = nv + stats->filledLoops;
    stats->outTriangles = nt + stats->filledEdges;
    stats->scaleExponent = e;
    if (stats->outVertices >= (uint64_t(1) << 32) || stats->outTriangles >= ((uint64_t(1) << 32) + 2) / 3)
        return setError(MLSGPU_ERR_LENGTH, "mesh fill holes: the filled mesh (%llu vertices, %llu triangles) does not fit 32-bit indices",
                        (unsigned long long) stats->outVertices, (unsigned long long) stats->outTriangles);
    if (capVertices < stats->outVertices || capTriangles < stats->outTriangles)
        return setError(MLSGPU_ERR_LENGTH, "mesh fill holes: the outputs hold %llu vertices and %llu triangles, the filled mesh has %llu and %llu",
                        (unsigned long long) capVertices, (unsigned long long) capTriangles, (unsigned long long) stats->outVertices,
                        (unsigned long long) stats->outTriangles);
    REQUIRE(stats->outVertices == 0 || dOutVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(stats->outTriangles == 0 || dOutTriangles != nullptr, MLSGPU_ERR_INVALID);

    if (nv > 0)
        HIP_CHECK(hipMemcpyAsync(dOutVertices, dVertices, nv * 12, hipMemcpyDeviceToDevice, ctx->stream));
    if (nt > 0)
        HIP_CHECK(hipMemcpyAsync(dOutTriangles, dTriangles, nt * 12, hipMemcpyDeviceToDevice, ctx->stream));
    if (stats->filledLoops > 0)
    {
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.fill.number", FilledRootIn{length.get(), flags.get(), maxEdges},
                                           NewVertexOut{length.get(), sums.get(), loopOf.get(), dOutVertices + 3 * nv, powerOfTwo(e - 30)},
                                           nv, 0u, tileSums.get(), (uint32_t *) nullptr)));
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.fill.emit",
                                           FilledVertexIn{outCount.get(), parent.get(), length.get(), flags.get(), maxEdges},
                                           NewTriangleOut{parent.get(), next.get(), loopOf.get(), dOutTriangles + 3 * nt, (uint32_t) nv},
                                           nv, 0u, tileSums.get(), (uint32_t *) nullptr)));
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));       /* the scratch goes with the call */
    return MLSGPU_OK;
}
