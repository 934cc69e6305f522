/*
 * Vertex-clustering simplification of an indexed triangle mesh that is resident in HBM.  The reference has no counterpart:
 * its meshes leave the device whole (src/mesher.cpp:763-852).  The contract (include/mlsgpu_hip.h, DESIGN.md "Mesh
 * simplification") is written so that every output is an integer or one correctly rounded operation away from integers: the
 * result does not depend on the schedule.
 *
 *   bounds     a thread per vertex: its cell per axis (f32), validity, the largest cell per axis     } one read-back: errors,
 *   indices    a thread per index: indices >= V are counted                                         } bits of the cell key
 *   keys       a thread per vertex: the cell key, packed into as many bits as the largest cells need
 *   sort       (key, vertex id) by key: a cluster becomes a run
 *   clusters   a scan over the run heads: the cluster of every vertex and of every sorted position, where each run starts
 *   sums       a thread per sorted position: 2^-30 fixed-point offsets inside the cell, added up per cluster in 64-bit integers
 *              (a wave that lies inside one cluster adds once, a cluster of one member adds nothing)
 *   map        a thread per triangle: its three clusters, collapsed or rotated so that the smallest comes first
 *   survivors  a scan that packs the surviving triangles: (third cluster, triangle id)
 *   sort       stable by the third cluster, then (pairs kernel) stable by first << b | second: (first, second, third) order
 *   unique     a scan over "differs from its predecessor": the kept triangles, as cluster triples, and the clusters they use
 *   vertices   a scan over the used clusters: the dense numbering, and the position of every used cluster
 *   reindex    a thread per output index: cluster -> output vertex
 *
 * An index >= V is compared and counted, never used as an address.
 *
 * Scratch belongs to the call: 60 bytes per vertex (the sort's two sides 24, cluster of a vertex 4, run starts 4, sums 24,
 * used / new index 4) and 44 bytes per triangle (cluster triple 12, the two sides of the 32-bit sort 16 and of the 64-bit
 * sort's keys 16), the sort's histogram (4 KB per 4096 elements of the larger of the two) and the scans' tile sums.
 */
#include "meshpost.hpp"

#include <cmath>

using namespace mlsgpu;

namespace
{

/* 64-bit counters, read back twice */
enum
{
    C_BAD_VERTICES = 0,
    C_BAD_INDICES = 1,
    C_COLLAPSED = 2,
    C_WORDS = 3
};
/* 32-bit words: the largest cell per axis, and the totals the scans leave */
enum
{
    W_MAX_CELL = 0,     /* [3] */
    W_CLUSTERS = 3,
    W_SURVIVORS = 4,
    W_OUT_TRIANGLES = 5,
    W_OUT_VERTICES = 6,
    W_WORDS = 7
};

const uint32_t DROPPED = 0xFFFFFFFFu;       /* first cluster of a triangle that takes no further part; clusters are < V < 2^32 - 1 */
const float CELL_LIMIT = 2097152.0f;        /* 2^21 */
const double FIXED_ONE = 1073741824.0;      /* 2^30 */

struct Frame
{
    float origin[3];
    float cellSize;
};

/* how the three cells share a key: x in the low bits */
struct KeyBits
{
    uint32_t x, y, z;
    __host__ __device__ __forceinline__ uint64_t pack(const uint32_t c[3]) const
    {
        return (uint64_t) c[2] << (x + y) | (uint64_t) c[1] << x | c[0];
    }
    __device__ __forceinline__ void unpack(uint64_t key, uint32_t c[3]) const
    {
        c[0] = (uint32_t) (key & ((uint64_t(1) << x) - 1));
        c[1] = (uint32_t) ((key >> x) & ((uint64_t(1) << y) - 1));
        c[2] = (uint32_t) (key >> (x + y));
    }
};

/* step 1 of the contract: c = floorf((p - origin) / cellSize) per axis, two correctly rounded f32 operations; false for a
 * non-finite coordinate or a cell outside [0, 2^21) */
__device__ __forceinline__ bool cellOf(const float p[3], const Frame &F, uint32_t c[3])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const float f = floorf((p[k] - F.origin[k]) / F.cellSize);
        const bool in = isfinite(p[k]) && f >= 0.0f && f < CELL_LIMIT;
        c[k] = in ? (uint32_t) f : 0u;
        ok = ok && in;
    }
    return ok;
}

/* Every lane of every wave stays to the end: waveMax needs the full wave. */
__global__ __launch_bounds__(256) void boundsKernel(const float *vertices, uint64_t numVertices, Frame F, Counter *counters, uint32_t *words)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < numVertices;
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (live)
    {
        p[0] = vertices[3 * v];
        p[1] = vertices[3 * v + 1];
        p[2] = vertices[3 * v + 2];
    }
    uint32_t c[3] = {0, 0, 0};
    const bool ok = !live || cellOf(p, F, c);
    tally(!ok, &counters[C_BAD_VERTICES]);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const uint32_t most = waveMax(live && ok ? c[k] : 0u);
        if (laneId() == 0 && most != 0)
            atomicMax(&words[W_MAX_CELL + k], most);
    }
}

__global__ __launch_bounds__(256) void indicesKernel(const uint32_t *indices, uint64_t numIndices, uint64_t numVertices, Counter *counters)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    tally(i < numIndices && indices[i] >= numVertices, &counters[C_BAD_INDICES]);
}

__global__ __launch_bounds__(256) void keysKernel(const float *vertices, uint64_t numVertices, Frame F, KeyBits bits, uint64_t *keys)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= numVertices)
        return;
    const float p[3] = {vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]};
    uint32_t c[3];
    cellOf(p, F, c);            /* every vertex is valid: the read-back behind boundsKernel said so */
    keys[v] = bits.pack(c);
}

/* ---- clusters: a scan over the heads of the sorted keys' runs ---- */
struct HeadIn
{
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return i == 0 || keys[i] != keys[i - 1] ? 1u : 0u; }
};
struct ClusterOut
{
    const uint32_t *sortedVertex;
    uint32_t *clusterOfVertex, *clusterOfPosition, *start;
    uint64_t numVertices;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t before, uint32_t head) const
    {
        const uint32_t cluster = before + head - 1;
        clusterOfVertex[sortedVertex[i]] = cluster;
        clusterOfPosition[i] = cluster;
        if (head)
            start[cluster] = (uint32_t) i;
        if (i + 1 == numVertices)
            start[cluster + 1] = (uint32_t) numVertices;
    }
};

/* step 3 of the contract, first half: q = llrint(((p - origin) / cellSize - c) * 2^30) in doubles, per axis */
__device__ __forceinline__ void fixedOffsets(const float p[3], const uint32_t c[3], const Frame &F, long long q[3])
{
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const double d = (double) p[k] - (double) F.origin[k];
        const double f = d / (double) F.cellSize - (double) c[k];
        q[k] = (long long) rint(f * FIXED_ONE);
    }
}

/* A thread per SORTED position, so that the members of a cluster are neighbours: a wave whose positions all lie in one
 * cluster (every wave but two of a large cluster) adds up in registers and issues three atomics; a cluster of one member
 * keeps its vertex and adds nothing.  No lane leaves early: the shuffles read every lane. */
__global__ __launch_bounds__(256) void sumsKernel(const float *vertices, const uint64_t *sortedKeys, const uint32_t *sortedVertex,
                                                  const uint32_t *clusterOfPosition, uint64_t numVertices, Frame F, KeyBits bits,
                                                  Counter *sums)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < numVertices;
    uint64_t key = 0, before = 0, after = 0;
    uint32_t v = 0, cluster = 0;
    if (live)
    {
        key = sortedKeys[i];
        before = i > 0 ? sortedKeys[i - 1] : ~key;
        after = i + 1 < numVertices ? sortedKeys[i + 1] : ~key;
        v = sortedVertex[i];
        cluster = clusterOfPosition[i];
    }
    const bool adds = live && (before == key || after == key);
    long long q[3] = {0, 0, 0};
    if (adds)
    {
        const float p[3] = {vertices[3 * (uint64_t) v], vertices[3 * (uint64_t) v + 1], vertices[3 * (uint64_t) v + 2]};
        uint32_t c[3];
        bits.unpack(key, c);
        fixedOffsets(p, c, F, q);
    }
    const uint64_t adders = __ballot(adds);
    if (adders == 0)
        return;                 /* (wave-uniform) */
    const uint32_t firstCluster = readLane(cluster, (int) __builtin_ctzll(adders));
    const bool oneCluster = __ballot(adds && cluster != firstCluster) == 0;
    if (oneCluster)
    {
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            const long long s = waveSum64(q[k]);        /* zero in the lanes that do not add */
            if (laneId() == 0)
                atomicAdd(&sums[3 * (uint64_t) firstCluster + k], (Counter) s);
        }
    }
    else if (adds)
    {
#pragma unroll
        for (int k = 0; k < 3; k++)
            atomicAdd(&sums[3 * (uint64_t) cluster + k], (Counter) q[k]);
    }
}

/* step 4, first half.  A triangle that collapses (or names a vertex that does not exist: counted before, never followed)
 * gets DROPPED as its first cluster. */
__global__ __launch_bounds__(256) void mapKernel(const uint32_t *triangles, uint64_t numTriangles, uint64_t numVertices,
                                                 const uint32_t *clusterOfVertex, uint32_t *mapped, Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint32_t i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
    const bool inRange = i0 < numVertices && i1 < numVertices && i2 < numVertices;
    uint32_t a = DROPPED, b = 0, c = 0;
    bool collapsed = false;
    if (inRange)
    {
        a = clusterOfVertex[i0];
        b = clusterOfVertex[i1];
        c = clusterOfVertex[i2];
        collapsed = a == b || b == c || c == a;
        if (collapsed)
            a = DROPPED;
        else if (b < a && b < c)
        {
            const uint32_t x = a;
            a = b; b = c; c = x;
        }
        else if (c < a && c < b)
        {
            const uint32_t x = a;
            a = c; c = b; b = x;
        }
    }
    tally(collapsed, &counters[C_COLLAPSED]);
    mapped[3 * t] = a;
    mapped[3 * t + 1] = b;
    mapped[3 * t + 2] = c;
}

struct SurvivorIn
{
    const uint32_t *mapped;
    __device__ __forceinline__ uint32_t operator()(uint64_t t) const { return mapped[3 * t] != DROPPED ? 1u : 0u; }
};
struct SurvivorOut
{
    const uint32_t *mapped;
    uint32_t *third, *id;
    __device__ __forceinline__ void operator()(uint64_t t, uint32_t before, uint32_t survives) const
    {
        if (survives)
        {
            third[before] = mapped[3 * t + 2];
            id[before] = (uint32_t) t;
        }
    }
};

/* between the two sorts: the survivors in the order of their third cluster get first << b | second as their key */
__global__ __launch_bounds__(256) void pairsKernel(const uint32_t *mapped, const uint32_t *id, const uint32_t *numSurvivors, uint32_t b,
                                                   uint64_t *keys)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *numSurvivors)
        return;
    const uint64_t t = id[i];
    keys[i] = (uint64_t) mapped[3 * t] << b | mapped[3 * t + 1];
}

/* the survivors in (first, second, third) order: one of a run of equal triples is kept */
struct UniqueIn
{
    const uint64_t *keys;
    const uint32_t *id, *mapped;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        if (i == 0)
            return 1u;
        const uint64_t key = keys[i], keyBefore = keys[i - 1];
        const uint64_t t = id[i], tBefore = id[i - 1];
        return key != keyBefore || mapped[3 * t + 2] != mapped[3 * tBefore + 2] ? 1u : 0u;
    }
};
struct UniqueOut
{
    const uint64_t *keys;
    const uint32_t *id, *mapped;
    uint32_t b;
    uint32_t *outTriangles, *used;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t before, uint32_t kept) const
    {
        if (!kept)
            return;
        const uint64_t key = keys[i];
        const uint32_t first = (uint32_t) (key >> b), second = (uint32_t) (key & ((uint64_t(1) << b) - 1));
        const uint32_t third = mapped[3 * (uint64_t) id[i] + 2];
        outTriangles[3 * (uint64_t) before] = first;
        outTriangles[3 * (uint64_t) before + 1] = second;
        outTriangles[3 * (uint64_t) before + 2] = third;
        used[first] = 1u;       /* plain stores that race only with stores of the same value */
        used[second] = 1u;
        used[third] = 1u;
    }
};

/* steps 3 (second half) and 5: the used clusters in key order are the output vertices */
struct UsedIn
{
    const uint32_t *used;
    __device__ __forceinline__ uint32_t operator()(uint64_t c) const { return used[c]; }
};
struct VertexOut
{
    const float *vertices;
    const uint64_t *sortedKeys;
    const uint32_t *sortedVertex, *start;
    const Counter *sums;
    Frame F;
    KeyBits bits;
    uint32_t *newIndex;         /* the array UsedIn reads: an element is read by the thread that writes it, before */
    float *outVertices;
    __device__ __forceinline__ void operator()(uint64_t cluster, uint32_t before, uint32_t isUsed) const
    {
        newIndex[cluster] = before;
        if (!isUsed)
            return;
        const uint32_t first = start[cluster], members = start[cluster + 1] - first;
        float out[3];
        if (members == 1)
        {
            const uint64_t v = sortedVertex[first];
#pragma unroll
            for (int k = 0; k < 3; k++)
                out[k] = vertices[3 * v + k];
        }
        else
        {
            uint32_t c[3];
            bits.unpack(sortedKeys[first], c);
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                const long long S = (long long) sums[3 * cluster + k];
                const double mean = ((double) S / (double) members) * (1.0 / FIXED_ONE);
                out[k] = (float) ((double) F.origin[k] + ((double) c[k] + mean) * (double) F.cellSize);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++)
            outVertices[3 * (uint64_t) before + k] = out[k];
    }
};

__global__ __launch_bounds__(256) void reindexKernel(uint32_t *outTriangles, const uint32_t *numOutTriangles, const uint32_t *newIndex)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * (uint64_t) *numOutTriangles)
        return;
    outTriangles[i] = newIndex[outTriangles[i]];
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_simplify(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                        uint64_t numTriangles, const float origin[3], float cellSize, float *dOutVertices,
                                        uint32_t *dOutTriangles, mlsgpu_simplify_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr && origin != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(cellSize) && cellSize > 0.0f, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), MLSGPU_ERR_INVALID);
    /* the sorts' values and tile counts are 32-bit, and so are the indices of a triangle */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || (dVertices != nullptr && dOutVertices != nullptr), MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || (dTriangles != nullptr && dOutTriangles != nullptr), MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->inVertices = numVertices;
    stats->inTriangles = numTriangles;
    if (numVertices == 0 && numTriangles == 0)
        return MLSGPU_OK;

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t nv = numVertices, nt = numTriangles, most = std::max(nv, nt);
    const Frame F = {{origin[0], origin[1], origin[2]}, cellSize};
    const dim3 B(256);
    DeviceArray<Counter> counters;
    DeviceArray<uint32_t> words;
    PROPAGATE(counters.alloc(C_WORDS));
    PROPAGATE(words.alloc(W_WORDS));
    HIP_CHECK(hipMemsetAsync(counters.get(), 0, C_WORDS * sizeof(Counter), ctx->stream));
    HIP_CHECK(hipMemsetAsync(words.get(), 0, W_WORDS * sizeof(uint32_t), ctx->stream));
    if (nv > 0)
        LAUNCH(ctx, "kernel.simplify.bounds", boundsKernel, dim3(divUp(nv, 256)), B, dVertices, nv, F, counters.get(), words.get());
    if (nt > 0)
        LAUNCH(ctx, "kernel.simplify.indices", indicesKernel, dim3(divUp(3 * nt, 256)), B, dTriangles, 3 * nt, nv, counters.get());
    Counter hCounters[C_WORDS];
    uint32_t hWords[W_WORDS];
    HIP_CHECK(hipMemcpyAsync(hCounters, counters.get(), sizeof(hCounters), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(hWords, words.get(), sizeof(hWords), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (hCounters[C_BAD_VERTICES] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh simplify: %llu vertices are not finite or lie outside the 2^21 cells per axis",
                        hCounters[C_BAD_VERTICES]);
    if (hCounters[C_BAD_INDICES] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh simplify: %llu triangle indices are out of range", hCounters[C_BAD_INDICES]);
    if (nv == 0 || nt == 0)
        return MLSGPU_OK;       /* an empty mesh */

    const KeyBits bits = {bitLength(hWords[W_MAX_CELL]), bitLength(hWords[W_MAX_CELL + 1]), bitLength(hWords[W_MAX_CELL + 2])};
    const uint32_t b = bitLength(nv);           /* a cluster is < V */
    DeviceArray<uint64_t> vKeysA, vKeysB, tKeysA, tKeysB;
    DeviceArray<uint32_t> vValsA, vValsB, hist, tileSums, clusterOfVertex, start, used, mapped, thirdA, thirdB, tValsA, tValsB;
    DeviceArray<Counter> sums;
    const uint64_t histElems = sortHistElems(most), tileElems = (uint64_t) scanTiles(most) + 1;
    PROPAGATE(vKeysA.alloc(nv));
    PROPAGATE(vKeysB.alloc(nv));
    PROPAGATE(vValsA.alloc(nv));
    PROPAGATE(vValsB.alloc(nv));
    PROPAGATE(clusterOfVertex.alloc(nv));
    PROPAGATE(start.alloc(nv + 1));
    PROPAGATE(sums.alloc(3 * nv));
    PROPAGATE(used.alloc(nv));
    PROPAGATE(mapped.alloc(3 * nt));
    PROPAGATE(thirdA.alloc(nt));
    PROPAGATE(thirdB.alloc(nt));
    PROPAGATE(tValsA.alloc(nt));
    PROPAGATE(tValsB.alloc(nt));
    PROPAGATE(tKeysA.alloc(nt));
    PROPAGATE(tKeysB.alloc(nt));
    PROPAGATE(hist.alloc(histElems));
    PROPAGATE(tileSums.alloc(tileElems));
    if (ctx->timing)
        ctx->addValue("simplify.scratch.bytes",
                      (double) (2 * vKeysA.bytes(nv) + 4 * vValsA.bytes(nv) + start.bytes(nv + 1) + sums.bytes(3 * nv)
                                + mapped.bytes(3 * nt) + 4 * thirdA.bytes(nt) + 2 * tKeysA.bytes(nt) + hist.bytes(histElems)
                                + tileSums.bytes(tileElems) + counters.bytes(C_WORDS) + words.bytes(W_WORDS)));
    uint32_t *const dWords = words.get();

    /* clusters */
    LAUNCH(ctx, "kernel.simplify.keys", keysKernel, dim3(divUp(nv, 256)), B, dVertices, nv, F, bits, vKeysA.get());
    SortResult<uint64_t> sv = {nullptr, nullptr};
    PROPAGATE(radixSort<uint64_t>(ctx, "kernel.simplify.sortVertices", vKeysA, vValsA, vKeysB, vValsB, nv, bits.x + bits.y + bits.z,
                                  true, hist, nullptr, &sv));
    /* the side of the sort that does not hold the result is free again: the cluster of every sorted position */
    uint32_t *const clusterOfPosition = sv.vals == vValsA.get() ? vValsB.get() : vValsA.get();
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.clusters", HeadIn{sv.keys},
                                       ClusterOut{sv.vals, clusterOfVertex, clusterOfPosition, start, nv}, nv, 0u, tileSums.get(),
                                       dWords + W_CLUSTERS)));
    HIP_CHECK(hipMemsetAsync(sums.get(), 0, 3 * nv * sizeof(Counter), ctx->stream));
    HIP_CHECK(hipMemsetAsync(used.get(), 0, nv * sizeof(uint32_t), ctx->stream));
    LAUNCH(ctx, "kernel.simplify.sums", sumsKernel, dim3(divUp(nv, 256)), B, dVertices, (const uint64_t *) sv.keys,
           (const uint32_t *) sv.vals, (const uint32_t *) clusterOfPosition, nv, F, bits, sums.get());

    /* triangles */
    LAUNCH(ctx, "kernel.simplify.map", mapKernel, dim3(divUp(nt, 256)), B, dTriangles, nt, nv, (const uint32_t *) clusterOfVertex.get(),
           mapped.get(), counters.get());
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.survivors", SurvivorIn{mapped}, SurvivorOut{mapped, thirdA, tValsA}, nt, 0u,
                                       tileSums.get(), dWords + W_SURVIVORS)));
    const uint32_t *const dSurvivors = dWords + W_SURVIVORS;
    SortResult<uint32_t> byThird = {nullptr, nullptr};
    PROPAGATE(radixSort<uint32_t>(ctx, "kernel.simplify.sortTriangles", thirdA, tValsA, thirdB, tValsB, nt, b, false, hist, nullptr,
                                  &byThird, dSurvivors));
    uint32_t *const idsOther = byThird.vals == tValsA.get() ? tValsB.get() : tValsA.get();
    LAUNCH(ctx, "kernel.simplify.pairs", pairsKernel, dim3(divUp(nt, 256)), B, (const uint32_t *) mapped.get(),
           (const uint32_t *) byThird.vals, dSurvivors, b, tKeysA.get());
    SortResult<uint64_t> ordered = {nullptr, nullptr};
    PROPAGATE(radixSort<uint64_t>(ctx, "kernel.simplify.sortTriangles", tKeysA.get(), byThird.vals, tKeysB.get(), idsOther, nt, 2 * b,
                                  false, hist, nullptr, &ordered, dSurvivors));
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.unique", UniqueIn{ordered.keys, ordered.vals, mapped},
                                       UniqueOut{ordered.keys, ordered.vals, mapped, b, dOutTriangles, used}, nt, 0u, tileSums.get(),
                                       dWords + W_OUT_TRIANGLES, dSurvivors)));

    /* output */
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.vertices", UsedIn{used},
                                       VertexOut{dVertices, sv.keys, sv.vals, start, sums, F, bits, used, dOutVertices}, nv, 0u,
                                       tileSums.get(), dWords + W_OUT_VERTICES, (const uint32_t *) (dWords + W_CLUSTERS))));
    LAUNCH(ctx, "kernel.simplify.reindex", reindexKernel, dim3(divUp(3 * nt, 256)), B, dOutTriangles,
           (const uint32_t *) (dWords + W_OUT_TRIANGLES), (const uint32_t *) used.get());

    HIP_CHECK(hipMemcpyAsync(hCounters, counters.get(), sizeof(hCounters), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(hWords, words.get(), sizeof(hWords), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    stats->outVertices = hWords[W_OUT_VERTICES];
    stats->outTriangles = hWords[W_OUT_TRIANGLES];
    stats->collapsedTriangles = hCounters[C_COLLAPSED];
    stats->duplicateTriangles = (uint64_t) hWords[W_SURVIVORS] - hWords[W_OUT_TRIANGLES];
    return MLSGPU_OK;
}
