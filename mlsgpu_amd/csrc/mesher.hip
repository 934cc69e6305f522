/*
 * Device-side mesh sink: what OOCMesher (src/mesher.cpp) does with the meshes Marching ships out -- weld of
 * external vertices by 64-bit key across buckets, connected components, pruning of components below a fraction
 * of the total vertex count, one output mesh per chunk -- for meshes that stay RESIDENT IN HBM.  Row f3 of
 * SURVEY.md section 8.
 *
 * The reference copies every ship-out to the host, runs a union-find per block plus a hash map of keys on ONE
 * mesher thread, spills to temporary files and re-reads them to write the PLY (src/mesher.cpp:220-469,763-852);
 * its manual names that thread as the scaling limit (doc/mlsgpu-user-manual.xml:508-511).  Here add() is a
 * device-to-device append of the DeviceKeyMesh into arenas (288 GB: the 13.5 GB mesh of the cfg3 noise cloud fits
 * many times) and finalize() is a handful of passes:
 *   1. externals: stable radix sort of (key, slot) -- blocks arrive grouped by chunk, so equal keys end up ordered
 *      by chunk; the first vertex of a key run is the vertex's identity for components (updateClumpKeyMap,
 *      :286-311), the first of a (key, chunk) run its identity in that chunk's file (externalRemap, :538-567);
 *   2. components: lock-free union-find over the triangles' two edges (computeLocalComponents uses the same two,
 *      :228-235) with CAS hooking, then full path compression;
 *   3. component sizes (each welded vertex once), the prune threshold uint64(total * threshold) and the
 *      keep test `>=` of getStatistics (:491-536);
 *   4. two scans compact the kept vertices and triangles; a chunk's indices are relative to its first vertex.
 * Output order is (chunk, block arrival, vertex / triangle order inside the block); the reference's differs
 * (clump order, reorder buffer) and its own tests compare up to isomorphism (test/test_mesher.cpp:401-460).
 */
#include "common.hpp"
#include "primitives.hpp"
#include "unionfind.hpp"

#include <algorithm>
#include <cstdlib>
#include <mutex>

using namespace mlsgpu;

namespace
{

struct MeshRecord
{
    uint64_t chunk;
    uint32_t vBase, nv, nInternal;
    uint64_t tBase, nt;
    uint32_t eBase;
};

/* per block, on the device: what the finalize kernels look up by binary search over tBase / vBase */
struct BlockTable
{
    const uint64_t *tBase;      /* [blocks + 1] */
    const uint32_t *vBase;      /* [blocks + 1] */
    const uint32_t *chunkOf;    /* [blocks] dense chunk index */
    const uint32_t *chunkVStart;/* [chunks + 1] output vertex index where the chunk starts (after the vertex scan) */
    uint32_t blocks;

    __device__ __forceinline__ uint32_t blockOfTriangle(uint64_t t) const
    {
        uint32_t lo = 0, hi = blocks;           /* last block with tBase <= t */
        while (hi - lo > 1)
        {
            const uint32_t mid = (lo + hi) >> 1;
            if (tBase[mid] <= t) lo = mid; else hi = mid;
        }
        return lo;
    }
};

__global__ void rebaseTrianglesKernel(uint32_t *tri, uint64_t n3, uint32_t base)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n3)
        tri[i] += base;
}

/* copy + rebase in one pass (same-device appends): four indices per thread */
__global__ __launch_bounds__(256) void copyRebaseTrianglesKernel(uint32_t *dst, const uint32_t *src, uint64_t n3, uint32_t base)
{
    const uint64_t i = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 4 <= n3 && ((((uintptr_t) dst) | ((uintptr_t) src)) & 15) == 0)
    {
        uint4 v = *reinterpret_cast<const uint4 *>(src + i);
        v.x += base; v.y += base; v.z += base; v.w += base;
        *reinterpret_cast<uint4 *>(dst + i) = v;
    }
    else
        for (uint64_t k = i; k < n3 && k < i + 4; k++)
            dst[k] = src[k] + base;
}

__global__ void fillExternalsKernel(uint32_t *gid, uint32_t *chunk, uint64_t n, uint32_t firstGid, uint32_t chunkIndex)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
    {
        gid[i] = firstGid + (uint32_t) i;
        chunk[i] = chunkIndex;
    }
}

__global__ void iotaKernel(uint32_t *a, uint64_t n)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        a[i] = (uint32_t) i;
}

/* externals sorted by key (ties in arrival = chunk order): identities of every external vertex */
__global__ void externalRepsKernel(const uint64_t *keys, const uint32_t *slots, const uint32_t *extGid, const uint32_t *extChunk,
                                   uint64_t n, uint32_t *compRep, uint32_t *outRep)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t key = keys[i];
    const uint32_t chunk = extChunk[slots[i]];
    uint64_t c = i, o = i;
    /* runs are as long as the number of blocks that share the vertex (at most 8 for bucket corners) */
    while (c > 0 && keys[c - 1] == key)
        c--;
    while (o > 0 && keys[o - 1] == key && extChunk[slots[o - 1]] == chunk)
        o--;
    const uint32_t g = extGid[slots[i]];
    compRep[g] = extGid[slots[c]];
    outRep[g] = extGid[slots[o]];
}

/* union of the endpoints of two edges per triangle (the third is redundant, src/mesher.cpp:231-234) */
__global__ void unionKernel(const uint32_t *tri, uint64_t nt, const uint32_t *compRep, uint32_t *parent, uint32_t *failed,
                            uint32_t shortcut)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt)
        return;
    const uint32_t v[3] = {compRep[tri[3 * t]], compRep[tri[3 * t + 1]], compRep[tri[3 * t + 2]]};
#pragma unroll
    for (int e = 0; e < 2; e++)
    {
        unite(parent, v[e], v[e + 1], failed, shortcut);
    }
}

__global__ void compressKernel(uint32_t *parent, const uint32_t *compRep, uint64_t n, uint32_t *root)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        root[i] = findRoot(parent, compRep[i]);
}

/* vertices of a component: every welded vertex once.  Neighbouring vertices mostly share their component (a noise
 * cloud is ONE component of hundreds of millions of vertices, and 6 million same-address atomics take 67 ms), so each
 * wave walks a contiguous span and keeps one pending (root, count) in registers; it only touches memory when the root
 * changes. */
#define SIZE_SPAN 64        /* steps of 64 vertices per wave */

/* The walk of the three counting kernels: a wave takes SIZE_SPAN steps of 64 items over [0, n); in a step the lanes whose item
 * countsAt(i) load valueAt(i), and sink(value, lanes) is called, wave-uniformly and lowest lane first, once per equal value. */
template<typename Counts, typename Value, typename Sink>
__device__ __forceinline__ void forEachRun(uint64_t n, Counts countsAt, Value valueAt, Sink &sink)
{
    const uint64_t wave = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t first = wave * (64 * SIZE_SPAN);
    for (uint32_t s = 0; s < SIZE_SPAN; s++)
    {
        const uint64_t i = first + (uint64_t) s * 64 + laneId();
        if (first + (uint64_t) s * 64 >= n)
            break;
        const bool counts = i < n && countsAt(i);
        const uint32_t mine = counts ? valueAt(i) : 0u;
        uint64_t todo = __ballot(counts);
        while (todo != 0)
        {
            const uint32_t r = readLane(mine, (int) __builtin_ctzll(todo));
            const uint64_t same = __ballot(counts && mine == r) & todo;
            sink(r, (uint32_t) __popcll(same));
            todo &= ~same;
        }
    }
}

struct PendingRun           /* the pending (root, count) of a wave; flush() once more at the end */
{
    uint32_t *total;
    uint32_t root = 0, count = 0;
    __device__ __forceinline__ void flush()
    {
        if (count != 0 && laneId() == 0)
            atomicAdd(&total[root], count);
        count = 0;
    }
    __device__ __forceinline__ void operator()(uint32_t r, uint32_t c)
    {
        if (r != root)
            flush();
        root = r;
        count += c;
    }
};

__global__ __launch_bounds__(256) void componentSizeKernel(const uint32_t *compRep, const uint32_t *root, uint64_t n, uint32_t *size)
{
    PendingRun pending{size};
    forEachRun(n, [&](uint64_t i) { return compRep[i] == (uint32_t) i; }, [&](uint64_t i) { return root[i]; }, pending);
    pending.flush();
}

/* [0] welded vertices, [1] components, [2] kept components, [3] kept vertices */
__global__ __launch_bounds__(256) void componentStatsKernel(const uint32_t *compRep, const uint32_t *root, const uint32_t *size,
                                                           uint64_t n, uint64_t threshold, unsigned long long *stats, int pass)
{
    /* grid-stride with per-thread sums, one atomic per wave at the end */
    unsigned long long reps = 0, comps = 0, kept = 0, keptV = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
    {
        const bool rep = compRep[i] == (uint32_t) i;
        if (pass == 0)
            reps += rep ? 1 : 0;
        else if (rep && root[i] == (uint32_t) i)
        {
            comps++;
            if (size[i] >= threshold)
            {
                kept++;
                keptV += size[i];
            }
        }
    }
    const unsigned long long vals[4] = {reps, comps, kept, keptV};
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        unsigned long long v = vals[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            v += __shfl_xor(v, d, 64);
        if (laneId() == 0 && v != 0)
            atomicAdd(&stats[k], v);
    }
}

struct KeepVertexIn
{
    const uint32_t *outRep, *root, *size;
    uint64_t threshold;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        return (outRep[i] == (uint32_t) i && size[root[i]] >= threshold) ? 1u : 0u;
    }
};

struct VertexOut
{
    const float *vertices;
    float *out;
    uint32_t *index;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t excl, uint32_t keep) const
    {
        index[i] = excl;
        if (keep)
        {
            out[3 * (uint64_t) excl + 0] = vertices[3 * i + 0];
            out[3 * (uint64_t) excl + 1] = vertices[3 * i + 1];
            out[3 * (uint64_t) excl + 2] = vertices[3 * i + 2];
        }
    }
};

struct KeepTriangleIn
{
    const uint32_t *tri, *root, *size;
    uint64_t threshold;
    __device__ __forceinline__ uint32_t operator()(uint64_t t) const
    {
        return size[root[tri[3 * t]]] >= threshold ? 1u : 0u;
    }
};

struct TriangleOut
{
    const uint32_t *tri, *outRep, *vIndex;
    BlockTable B;
    uint32_t *out;
    __device__ __forceinline__ void operator()(uint64_t t, uint32_t excl, uint32_t keep) const
    {
        if (!keep)
            return;
        const uint32_t first = B.chunkVStart[B.chunkOf[B.blockOfTriangle(t)]];
#pragma unroll
        for (int j = 0; j < 3; j++)
            out[3 * (uint64_t) excl + j] = vIndex[outRep[tri[3 * t + j]]] - first;
    }
};

struct TriangleOutIdx
{
    TriangleOut inner;
    uint32_t *tIndex;
    __device__ __forceinline__ void operator()(uint64_t t, uint32_t excl, uint32_t keep) const
    {
        tIndex[t] = excl;
        inner(t, excl, keep);
    }
};

__global__ void gatherU32Kernel(const uint32_t *src, const uint64_t *at, uint32_t n, uint64_t limit, uint32_t last, uint32_t *dst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        dst[i] = at[i] < limit ? src[at[i]] : last;
}

/* ---- boundary export for several meshers, one job (see mlsgpu_hip_mesher_boundary) ---- */

/* the roots of the components, densely numbered in vertex order */
struct IsRootIn
{
    const uint32_t *compRep, *root;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        return (compRep[i] == (uint32_t) i && root[i] == (uint32_t) i) ? 1u : 0u;
    }
};
struct RootOut
{
    uint32_t *rootId, *denseOf;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t excl, uint32_t isRoot) const
    {
        denseOf[i] = excl;
        if (isRoot)
            rootId[excl] = (uint32_t) i;
    }
};

/* triangles per component, by the span trick of componentSizeKernel (a noise cloud is one component) */
__global__ __launch_bounds__(256) void componentTrianglesKernel(const uint32_t *tri, const uint32_t *root, const uint32_t *denseOf,
                                                                uint64_t nt, uint32_t *count)
{
    PendingRun pending{count};
    forEachRun(nt, [](uint64_t) { return true; }, [&](uint64_t t) { return denseOf[root[tri[3 * t]]]; }, pending);
    pending.flush();
}

/* The same count for FEW components (surface-like data: a handful of sheets whose triangles alternate along every row of
 * cells, so the run-length trick above flushes at almost every step and a million global atomics land on a dozen
 * addresses): per-workgroup bins in LDS, one global atomic per bin and workgroup. */
#define FEW_COMPONENTS 2048
__global__ __launch_bounds__(256) void componentTrianglesFewKernel(const uint32_t *tri, const uint32_t *root, const uint32_t *denseOf,
                                                                   uint64_t nt, uint32_t numRoots, uint32_t *count)
{
    __shared__ uint32_t bins[FEW_COMPONENTS];
    for (uint32_t d = threadIdx.x; d < numRoots; d += 256)
        bins[d] = 0;
    __syncthreads();
    auto toBin = [&](uint32_t r, uint32_t c) { if (laneId() == 0) atomicAdd(&bins[r], c); };
    forEachRun(nt, [](uint64_t) { return true; }, [&](uint64_t t) { return denseOf[root[tri[3 * t]]]; }, toBin);
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < numRoots; d += 256)
        if (bins[d] != 0)
            atomicAdd(&count[d], bins[d]);
}

__global__ void gatherSizesKernel(const uint32_t *rootId, const uint32_t *size, uint32_t n, uint32_t *out)
{
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < n)
        out[d] = size[rootId[d]];
}

/* every distinct external key (the keys are sorted) with the dense root of its vertex */
struct FirstOfRunIn
{
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return (i == 0 || keys[i - 1] != keys[i]) ? 1u : 0u; }
};
struct KeyRootOut
{
    const uint64_t *keys;
    const uint32_t *slots, *extGid, *root, *denseOf;
    uint64_t *keyOut;
    uint32_t *rootOut;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t excl, uint32_t first) const
    {
        if (first)
        {
            keyOut[excl] = keys[i];
            rootOut[excl] = denseOf[root[extGid[slots[i]]]];
        }
    }
};

/* the caller's verdict per dense root becomes the "size" the output pass tests against a threshold of 1 */
__global__ void applyVerdictKernel(const uint32_t *rootId, const uint8_t *keep, uint32_t n, uint32_t *size)
{
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < n)
        size[rootId[d]] = keep[d] ? 0xFFFFFFFFu : 0u;
}

template<typename T>
struct Arena
{
    DeviceArray<T> ptr;
    uint64_t used = 0;
    uint64_t cap() const { return ptr.capacity(); }

    /* the mesher's device must be current; `stream` is one of its streams */
    int reserve(hipStream_t stream, uint64_t need)
    {
        if (need <= cap())
            return MLSGPU_OK;
        DeviceArray<T> grown;
        PROPAGATE(grown.alloc(std::max<uint64_t>(need, cap() + cap() / 2 + 1024)));
        if (used > 0)
        {
            hipError_t e = hipMemcpyAsync(grown, ptr, used * sizeof(T), hipMemcpyDeviceToDevice, stream);
            if (e == hipSuccess)
                e = hipStreamSynchronize(stream);
            if (e != hipSuccess)
                return setError(MLSGPU_ERR_HIP, "mesher: arena move failed: %s", hipGetErrorString(e));
        }
        ptr = std::move(grown);         /* the old buffer goes with `grown` */
        return MLSGPU_OK;
    }
};

const dim3 B(256);          /* every launch of the stages below */

/* bump allocator over a slab the mesher keeps between calls: allocating and freeing tens of GB of scratch costs
 * several times the kernels that use it.  Without a base it only measures: nothing is handed out, `used` adds up. */
struct Scratch
{
    char *base;
    uint64_t cap, used = 0;
    explicit Scratch(void *base = nullptr, uint64_t cap = ~uint64_t(0)) : base(static_cast<char *>(base)), cap(cap) {}
    template<typename T> int get(T **p, uint64_t n)
    {
        const uint64_t bytes = (std::max<uint64_t>(n, 1) * sizeof(T) + 255) & ~uint64_t(255);
        if (bytes > cap - used)
            return setError(MLSGPU_ERR_NOMEM, "mesher: scratch slab too small (%llu of %llu bytes used, %llu more wanted)",
                            (unsigned long long) used, (unsigned long long) cap, (unsigned long long) bytes);
        *p = base != nullptr ? reinterpret_cast<T *>(base + used) : nullptr;
        used += bytes;
        return MLSGPU_OK;
    }
};

struct SinkSizes
{
    uint64_t nv, nt, ne;        /* vertices, triangles and external vertices in the arenas */
    uint32_t nb, nc;            /* blocks, chunks */
    bool empty() const { return nv == 0 || nt == 0; }
};

/* Every array that finalize, boundary and finalize_with take from the slab, for all of them at once: where an array lies
 * depends on the five sizes alone.  That is what lets a call start from what an earlier one left behind (SinkCache). */
struct SinkScratch
{
    /* per vertex: the first of its key run and of its (key, chunk) run, the forest, its root, a root's vertices, its output index */
    uint32_t *compRep, *outRep, *parent, *root, *size, *vIndex;
    uint64_t *keysA, *keysB;                    /* the key sort's two halves ... */
    uint32_t *slotsA, *slotsB, *hist, *sortTileSums;
    bool sortedInA;                             /* ... and which of them holds the sorted keys (weld, or the cache) */
    uint32_t *dFailed, *dRootTotal, *rootTiles; /* the union did not converge; numberRoots */
    uint32_t *tcount, *vcount, *dKeyTotal, *keyTiles;   /* exportBoundary: triangles and vertices per root ([nv]: its bound) */
    uint8_t *dKeep;                             /* applyVerdict ([nv] likewise) */
    unsigned long long *dStats;                 /* writeOutput */
    uint64_t *dTBase, *dAt;
    uint32_t *dVBase, *dChunkOf, *dChunkVStart, *dChunkTStart, *dTotals, *tileSums, *tIndex;

    /* overlays.  From numberRoots on: root d's vertex, over the forest, which nothing reads once `root` is written ... */
    uint32_t *rootId() const { return parent; }
    /* ... and a root vertex's dense number, until writeOutput puts the output indices there */
    uint32_t *denseOf() const { return vIndex; }
    uint64_t *sortedKeys() const { return sortedInA ? keysA : keysB; }
    uint32_t *sortedSlots() const { return sortedInA ? slotsA : slotsB; }
    /* in exportBoundary: the distinct keys and their roots, over the halves the sort left free */
    uint64_t *keyOut() const { return sortedInA ? keysB : keysA; }
    uint32_t *rootOut() const { return sortedInA ? slotsB : slotsA; }

    int lay(Scratch &S, const SinkSizes &z)
    {
        for (uint32_t **p : {&compRep, &outRep, &parent, &root, &size, &vIndex, &tcount, &vcount})
            PROPAGATE(S.get(p, z.nv));
        PROPAGATE(S.get(&dKeep, z.nv));
        for (uint64_t **p : {&keysA, &keysB})
            PROPAGATE(S.get(p, z.ne));
        for (uint32_t **p : {&slotsA, &slotsB})
            PROPAGATE(S.get(p, z.ne));
        PROPAGATE(S.get(&hist, sortHistElems(z.ne)));
        PROPAGATE(S.get(&sortTileSums, scanTiles(std::max<uint64_t>(sortHistElems(z.ne), z.ne))));
        for (uint32_t **p : {&dFailed, &dRootTotal, &dKeyTotal})
            PROPAGATE(S.get(p, 1));
        PROPAGATE(S.get(&rootTiles, scanTiles(z.nv)));
        PROPAGATE(S.get(&keyTiles, scanTiles(z.ne)));
        PROPAGATE(S.get(&dStats, 4));
        PROPAGATE(S.get(&dTBase, z.nb + 1));
        PROPAGATE(S.get(&dVBase, z.nb + 1));
        PROPAGATE(S.get(&dChunkOf, z.nb));
        for (uint32_t **p : {&dChunkVStart, &dChunkTStart})
            PROPAGATE(S.get(p, z.nc + 1));
        PROPAGATE(S.get(&dAt, z.nc + 1));
        PROPAGATE(S.get(&dTotals, 2));
        PROPAGATE(S.get(&tileSums, scanTiles(std::max(z.nv, z.nt))));
        return S.get(&tIndex, z.nt);
    }
};

/* what the layout takes, and 1 MiB */
uint64_t scratchBytes(const SinkSizes &z)
{
    Scratch measure;
    SinkScratch L;
    (void) L.lay(measure, z);
    return measure.used + (1 << 20);
}

/* What the last analysis left in the slab, valid while nothing is added (same arenas) and the slab stays where it is.
 * AfterExport: boundary()'s weld and components (representatives, roots, sizes) AND the dense root numbering -- a
 * finalize_with() right behind it starts from them instead of sorting and uniting again (once: the verdict overwrites the
 * sizes).  AfterFinalize: finalize()'s weld and components (the output pass only rewrote the vertex index array) -- a
 * boundary() behind it numbers the roots and exports, without the key sort and the union-find. */
struct SinkCache
{
    enum Kind { None, AfterExport, AfterFinalize } kind = None;
    bool sortedInA = false;
    uint64_t nv = 0, nt = 0, ne = 0;
    uint32_t rootCount = 0;
    bool matches(uint64_t v, uint64_t t, uint64_t e) const { return kind != None && nv == v && nt == t && ne == e; }
    void drop() { kind = None; }
};
} // namespace

struct mlsgpu_mesher
{
    mlsgpu_ctx *ctx = nullptr;
    std::mutex mutex;
    double pruneThreshold = 0.0;
    bool background = false;        /* finalize shares the GPU with other work: see the union-find launch */
    Arena<float> vertices;          /* 3 per vertex */
    Arena<uint32_t> triangles;      /* 3 per triangle, global vertex ids */
    Arena<uint64_t> extKeys;
    Arena<uint32_t> extGid, extChunk;
    std::vector<MeshRecord> blocks;
    std::vector<uint64_t> chunkIds;             /* dense index -> caller's id, arrival order */
    bool finalized = false;
    bool peerEnabled[16] = {};                  /* peer access towards the GPUs whose workers have appended */
    SinkCache cache;                            /* what the last analysis left in the slab */
    /* results */
    DeviceArray<float> outVertices;             /* 3 per vertex */
    DeviceArray<uint32_t> outTriangles;         /* 3 per triangle */
    std::vector<uint64_t> chunkVStart, chunkTStart;     /* [chunks + 1] */
    std::vector<uint32_t> outChunks;                    /* dense chunk indices that have triangles */
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    /* vertex normals (mlsgpu_hip_mesher_chunk_normals): beside outVertices, a chunk's filled at its first request; whatever
     * changes the outputs empties normalsOf */
    DeviceArray<float> outNormals;              /* 3 per vertex */
    std::vector<char> normalsReady;             /* per dense chunk */
    std::vector<mlsgpu_normals_stats> normalsOf;
    /* the kept reference (mlsgpu_hip_mesher_keep_reference): a copy of the results as they were, with its own chunk tables */
    bool referenceKept = false;
    DeviceArray<float> refVertices;             /* 3 per vertex */
    DeviceArray<uint32_t> refTriangles;         /* 3 per triangle */
    std::vector<uint64_t> refVStart, refTStart; /* [chunks + 1] */
    void dropReference()
    {
        referenceKept = false;
        refVertices.release();
        refTriangles.release();
        refVStart.clear();
        refTStart.clear();
    }
    /* boundary export (mlsgpu_hip_mesher_boundary): valid until the next add */
    bool analyzed = false;
    /* the export's keys and their roots land in PINNED memory (tens of MB: a copy into pageable memory goes through the
     * runtime's staging buffers and took anything from 5 to 80 ms) */
    PinnedArray<uint64_t> bKeys;
    PinnedArray<uint32_t> bKeyRoot;
    std::vector<uint64_t> bRootVertices, bRootTriangles;

    /* kept between finalize calls; grown on demand (or up front by reserve) */
    DeviceArray<char> slab;

    int ensureSlab(uint64_t bytes)
    {
        if (bytes <= slab.capacity())
            return MLSGPU_OK;
        cache.drop();           /* whatever an analysis left in the old slab is gone */
        return slab.reserve(bytes);
    }
    int ensureOutputs(uint64_t nv, uint64_t nt)
    {
        PROPAGATE(outVertices.reserve(std::max<uint64_t>(3 * nv, 1)));
        return outTriangles.reserve(std::max<uint64_t>(3 * nt, 1));
    }
    /* a stream of the mesher's own: add() is called from worker threads whose contexts (and devices) differ, and the
     * mesher's context belongs to the thread that finalizes; everything on it runs under the mutex */
    hipStream_t addStream = nullptr;
    int ensureAddStream()
    {
        if (addStream == nullptr)
            HIP_CHECK(hipStreamCreateWithFlags(&addStream, hipStreamNonBlocking));
        return MLSGPU_OK;
    }
    /* appends that are still running on their producers' streams (same-device appends do not wait on the host: the
     * producer's next kernels are behind the copies in stream order).  Waited for before an arena moves, before any
     * analysis and before a reset. */
    struct PendingAppend
    {
        int device;
        hipEvent_t done;
    };
    std::vector<PendingAppend> pending, eventPool;
    int takeEvent(int device, hipEvent_t *ev)      /* `device` is current */
    {
        for (size_t i = 0; i < eventPool.size(); i++)
            if (eventPool[i].device == device)
            {
                *ev = eventPool[i].done;
                eventPool.erase(eventPool.begin() + (long) i);
                return MLSGPU_OK;
            }
        HIP_CHECK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
        return MLSGPU_OK;
    }
    int drainPending(size_t keep = 0)
    {
        while (pending.size() > keep)
        {
            const hipError_t e = hipEventSynchronize(pending.front().done);
            eventPool.push_back(pending.front());
            pending.erase(pending.begin());
            if (e != hipSuccess)
                return setError(MLSGPU_ERR_HIP, "mesher: an append failed: %s", hipGetErrorString(e));
        }
        return MLSGPU_OK;
    }
    int regroupByChunk();
    struct Span { uint64_t v0, t0, nv, nt; };
    Span span(size_t c) const           /* dense chunk c of the results: first vertex and triangle, how many of each */
    {
        return {chunkVStart[c], chunkTStart[c], chunkVStart[c + 1] - chunkVStart[c], chunkTStart[c + 1] - chunkTStart[c]};
    }
    void dropNormals() { normalsReady.clear(); }
    void dropResults() { finalized = false; dropNormals(); }
    int chunkNormals(uint32_t c, const float **dNormals, mlsgpu_normals_stats *out);
    /* finalize, boundary and finalize_with: a shared start, then their stages in this order */
    int begin(SinkSizes &z, SinkScratch &L, SinkCache &had);
    int weld(SinkScratch &L, const SinkSizes &z);
    int components(const SinkScratch &L, const SinkSizes &z);
    /* weld and components, unless the slab still holds them; the union's failure flag is cleared either way */
    int analyse(SinkScratch &L, const SinkSizes &z, bool cached)
    {
        if (!cached)
            PROPAGATE(weld(L, z));
        HIP_CHECK(hipMemsetAsync(L.dFailed, 0, 4, ctx->stream));
        return cached ? MLSGPU_OK : components(L, z);
    }
    int checkUnion(const SinkScratch &L)        /* the union's failure flag, behind whatever is on the stream: synchronises */
    {
        uint32_t hFailed = 0;
        HIP_CHECK(hipMemcpyAsync(&hFailed, L.dFailed, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (hFailed != 0)
            return setError(MLSGPU_ERR_HIP, "mesher: component union did not converge");
        return MLSGPU_OK;
    }
    int numberRoots(const SinkScratch &L, const SinkSizes &z, uint32_t *rootCount);
    int exportBoundary(const SinkScratch &L, const SinkSizes &z, uint32_t rootCount);
    int applyVerdict(const SinkScratch &L, uint32_t rootCount, const uint8_t *keepRoots, uint64_t numRoots);
    int writeOutput(const SinkScratch &L, const SinkSizes &z, double fraction, uint64_t minSize);
    int finish(uint32_t *numChunks)             /* finalized, with the chunks writeOutput left (none for an empty sink) */
    {
        finalized = true;
        if (referenceKept && refVStart.size() != chunkVStart.size())
            dropReference();    /* another chunk list: the kept chunks no longer pair with these */
        if (numChunks)
            *numChunks = (uint32_t) outChunks.size();
        return MLSGPU_OK;
    }
    ~mlsgpu_mesher()
    {
        if (addStream) hipStreamDestroy(addStream);
        drainPending();
        for (auto &e : eventPool)
            hipEventDestroy(e.done);
    }
};

MLSGPU_API int mlsgpu_hip_mesher_create(mlsgpu_ctx *ctx, mlsgpu_mesher **out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    mlsgpu_mesher *m = new mlsgpu_mesher;
    m->ctx = ctx;
    *out = m;
    return MLSGPU_OK;
}

MLSGPU_API void mlsgpu_hip_mesher_destroy(mlsgpu_mesher *m) { delete m; }

/* on = 1: this sink's finalize usually runs while other work (the next job's buckets) is on the GPU: its union-find pass
 * holds back to a quarter of the wave slots.  Shells cloud, jobs in rotation: 40.6 -> 37.1 ms per job (the ship-out route:
 * 36.3); a finalize that has the GPU to itself takes 11-14 ms either way, the noise cloud's (378 M vertices) 97 -> 108 ms. */
MLSGPU_API int mlsgpu_hip_mesher_set_background(mlsgpu_mesher *m, int on)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    m->background = on != 0;
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesher_set_prune_threshold(mlsgpu_mesher *m, double threshold)
{
    REQUIRE(m != nullptr && threshold >= 0.0 && threshold <= 1.0, MLSGPU_ERR_INVALID);
    m->pruneThreshold = threshold;
    return MLSGPU_OK;
}

/* room for the whole job up front: an arena that has to grow is reallocated and copied */
MLSGPU_API int mlsgpu_hip_mesher_reserve(mlsgpu_mesher *m, uint64_t numVertices, uint64_t numTriangles, uint64_t numExternal)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    HIP_CHECK(hipSetDevice(m->ctx->device));
    PROPAGATE(m->ensureAddStream());
    /* an arena that grows moves (copy on addStream, old buffer freed): same-device appends may still be running on their
     * producers' streams, so they must have landed first -- the rule mlsgpu_hip_mesher_add follows before it grows one */
    if (3 * numVertices > m->vertices.cap() || 3 * numTriangles > m->triangles.cap() || numExternal > m->extKeys.cap()
        || numExternal > m->extGid.cap() || numExternal > m->extChunk.cap())
        PROPAGATE(m->drainPending());
    PROPAGATE(m->vertices.reserve(m->addStream, 3 * numVertices));
    PROPAGATE(m->triangles.reserve(m->addStream, 3 * numTriangles));
    PROPAGATE(m->extKeys.reserve(m->addStream, numExternal));
    PROPAGATE(m->extGid.reserve(m->addStream, numExternal));
    PROPAGATE(m->extChunk.reserve(m->addStream, numExternal));
    /* finalize's scratch and outputs too (a few hundred blocks and chunks are assumed; finalize grows it otherwise) */
    PROPAGATE(m->ensureSlab(scratchBytes(SinkSizes{numVertices, numTriangles, numExternal, 4096, 4096})));
    PROPAGATE(m->ensureOutputs(numVertices, numTriangles));
    return MLSGPU_OK;
}

/* MesherBase::InputFunctor (src/mesher.h:204-210) for a mesh that is still on a device */
MLSGPU_API int mlsgpu_hip_mesher_add(mlsgpu_mesher *m, mlsgpu_ctx *from, uint64_t chunkId, const mlsgpu_mesh *mesh)
{
    REQUIRE(m != nullptr && from != nullptr && mesh != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(mesh->numInternalVertices <= mesh->numVertices, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(!m->finalized, MLSGPU_ERR_INVALID);
    const int home = m->ctx->device;
    static const bool forcePeer = [] {          /* tests: the peer route on one GPU; said once, it synchronises every append */
        const bool on = getenv("MLSGPU_HIP_MESHER_FORCE_PEER") != nullptr;
        if (on)
            fprintf(stderr, "mlsgpu_hip: MLSGPU_HIP_MESHER_FORCE_PEER is set: ship-outs take the peer route (test hook)\n");
        return on;
    }();
    const bool peer = from->device != home || forcePeer;
    DeviceGuard restore;        /* the caller is a worker in the middle of ITS device's work (Marching's output functor) */
    if (from->device != home && !m->peerEnabled[from->device & 15])
    {
        enablePeerAccess(home, from->device);
        m->peerEnabled[from->device & 15] = true;
    }
    HIP_CHECK(hipSetDevice(home));
    PROPAGATE(m->ensureAddStream());
    /* OOCMesher::add indexes chunks[chunkId.gen] (src/mesher.cpp:380-384): any arrival order; dense index = first arrival */
    uint32_t chunk = 0;
    while (chunk < m->chunkIds.size() && m->chunkIds[chunk] != chunkId)
        chunk++;
    const bool newChunk = chunk == m->chunkIds.size();     /* recorded with the block, once everything has succeeded */
    const uint64_t nv = mesh->numVertices, nt = mesh->numTriangles, ne = nv - mesh->numInternalVertices;
    REQUIRE(m->vertices.used / 3 + nv < (uint64_t(1) << 32), MLSGPU_ERR_LENGTH);
    /* an arena that has to grow moves: every earlier append must have landed first (reserve() up front avoids both) */
    if (m->vertices.used + 3 * nv > m->vertices.cap() || m->triangles.used + 3 * nt > m->triangles.cap()
        || m->extKeys.used + ne > m->extKeys.cap() || m->extGid.used + ne > m->extGid.cap() || m->extChunk.used + ne > m->extChunk.cap())
        PROPAGATE(m->drainPending());
    PROPAGATE(m->vertices.reserve(m->addStream, m->vertices.used + 3 * nv));
    PROPAGATE(m->triangles.reserve(m->addStream, m->triangles.used + 3 * nt));
    PROPAGATE(m->extKeys.reserve(m->addStream, m->extKeys.used + ne));
    PROPAGATE(m->extGid.reserve(m->addStream, m->extGid.used + ne));
    PROPAGATE(m->extChunk.reserve(m->addStream, m->extChunk.used + ne));
    MeshRecord r;
    r.chunk = chunk;
    r.vBase = (uint32_t) (m->vertices.used / 3);
    r.nv = (uint32_t) nv;
    r.nInternal = (uint32_t) mesh->numInternalVertices;
    r.tBase = m->triangles.used / 3;
    r.nt = nt;
    r.eBase = (uint32_t) m->extKeys.used;
    /* the copies run on the producing worker's stream, behind the kernels that made the mesh; from another GPU they are
     * peer copies over the fabric.  The index fix-ups run on the mesher's device, after the copies. */
    HIP_CHECK(hipSetDevice(from->device));
    auto append = [&](void *dst, const void *src, size_t bytes) -> hipError_t
    {
        if (bytes == 0)
            return hipSuccess;
        return peer ? hipMemcpyPeerAsync(dst, home, src, from->device, bytes, from->stream)
                    : hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, from->stream);
    };
    /* A failure after the first enqueue leaves work on the producer's stream that writes [used, used + n) of the arenas
     * while `used` does not advance: the next append (possibly from another worker's stream) would write the same range
     * under it, and finalize / reset would not wait for it.  Every failing path therefore drains the producer's stream
     * (and the mesher's, for a peer append) before it reports. */
    hipStream_t fix = from->stream;
    auto enqueue = [&]() -> int
    {
        HIP_CHECK(append(m->vertices.ptr + m->vertices.used, mesh->dVertices, 3 * nv * sizeof(float)));
        if (peer)
            HIP_CHECK(append(m->triangles.ptr + m->triangles.used, mesh->dTriangles, 3 * nt * sizeof(uint32_t)));
        else if (nt > 0)
            hipLaunchKernelGGL(copyRebaseTrianglesKernel, dim3(divUp(divUp(3 * nt, 4), 256)), dim3(256), 0, from->stream,
                               m->triangles.ptr + m->triangles.used, mesh->dTriangles, 3 * nt, (uint32_t) (m->vertices.used / 3));
        HIP_CHECK(append(m->extKeys.ptr + m->extKeys.used, mesh->dVertexKeys + mesh->numInternalVertices, ne * sizeof(uint64_t)));
        if (peer)
        {
            HIP_CHECK(hipStreamSynchronize(from->stream));
            HIP_CHECK(hipSetDevice(home));
            fix = m->addStream;
        }
        if (nt > 0 && peer)
            hipLaunchKernelGGL(rebaseTrianglesKernel, dim3(divUp(3 * nt, 256)), dim3(256), 0, fix,
                               m->triangles.ptr + m->triangles.used, 3 * nt, r.vBase);
        if (ne > 0)
            hipLaunchKernelGGL(fillExternalsKernel, dim3(divUp(ne, 256)), dim3(256), 0, fix,
                               m->extGid.ptr + m->extGid.used, m->extChunk.ptr + m->extChunk.used, ne, r.vBase + r.nInternal, chunk);
        HIP_CHECK(hipGetLastError());
        return MLSGPU_OK;
    };
    {
        const int rcEnqueue = enqueue();
        if (rcEnqueue != MLSGPU_OK)
        {
            (void) hipStreamSynchronize(from->stream);
            if (fix != from->stream)
                (void) hipStreamSynchronize(fix);
            return rcEnqueue;
        }
    }
    if (peer)
    {
        /* the fix-ups ran on the mesher's stream, not the producer's: the mesh is Marching's and is reused for the next
         * ship-out, so they must have finished */
        HIP_CHECK(hipStreamSynchronize(fix));
    }
    else
    {
        /* same device: copies and fix-ups are on the PRODUCER's stream, ahead of whatever it does to the mesh next -- the
         * worker goes on without waiting; the mesher remembers that this append is still in flight */
        mlsgpu_mesher::PendingAppend p{from->device, nullptr};
        PROPAGATE(m->takeEvent(from->device, &p.done));
        if (hipEventRecord(p.done, fix) != hipSuccess)
        {
            m->eventPool.push_back(p);
            HIP_CHECK(hipStreamSynchronize(fix));
        }
        else
        {
            m->pending.push_back(p);
            PROPAGATE(m->drainPending(512));       /* bounds the list on jobs of thousands of ship-outs */
        }
    }
    m->vertices.used += 3 * nv;
    m->triangles.used += 3 * nt;
    m->extKeys.used += ne;
    m->extGid.used += ne;
    m->extChunk.used += ne;
    if (newChunk)
        m->chunkIds.push_back(chunkId);
    m->blocks.push_back(r);
    m->analyzed = false;
    m->cache.drop();
    return MLSGPU_OK;
}

/* a mlsgpu_farm_output_fn whose `user` is the mesher: the farm's device workers append their ship-outs */
MLSGPU_API int mlsgpu_hip_mesher_farm_output(void *mesher, int device, uint64_t chunkId, mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh)
{
    (void) device;
    return mlsgpu_hip_mesher_add(static_cast<mlsgpu_mesher *>(mesher), ctx, chunkId, mesh);
}

/* empties the mesher (arenas, scratch and outputs keep their capacity): the next job starts from nothing */
MLSGPU_API int mlsgpu_hip_mesher_reset(mlsgpu_mesher *m)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    PROPAGATE(m->drainPending());
    m->vertices.used = m->triangles.used = 0;
    m->extKeys.used = m->extGid.used = m->extChunk.used = 0;
    m->blocks.clear();
    m->chunkIds.clear();
    m->outChunks.clear();
    m->dropResults();
    m->dropReference();
    m->analyzed = false;
    m->cache.drop();
    return MLSGPU_OK;
}

/* finalize wants the blocks of a chunk adjacent in the arenas (output order is arena order, and equal keys must sort by
 * chunk).  With several workers and several chunks they arrive interleaved: move the blocks into (chunk by first
 * arrival, arrival) order -- device-to-device copies into fresh arenas, vertex ids shifted by the block's move. */
int mlsgpu_mesher::regroupByChunk()
{
    bool grouped = true;
    for (size_t b = 1; b < blocks.size(); b++)
        grouped = grouped && blocks[b - 1].chunk <= blocks[b].chunk;
    if (grouped)
        return MLSGPU_OK;
    std::vector<uint32_t> order(blocks.size());
    for (uint32_t i = 0; i < order.size(); i++)
        order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return blocks[a].chunk < blocks[b].chunk; });
    PROPAGATE(ensureAddStream());
    Arena<float> nVertices;
    Arena<uint32_t> nTriangles, nGid, nChunk;
    Arena<uint64_t> nKeys;
    PROPAGATE(nVertices.reserve(addStream, std::max<uint64_t>(vertices.cap(), 1)));
    PROPAGATE(nTriangles.reserve(addStream, std::max<uint64_t>(triangles.cap(), 1)));
    PROPAGATE(nKeys.reserve(addStream, std::max<uint64_t>(extKeys.cap(), 1)));
    PROPAGATE(nGid.reserve(addStream, std::max<uint64_t>(extGid.cap(), 1)));
    PROPAGATE(nChunk.reserve(addStream, std::max<uint64_t>(extChunk.cap(), 1)));
    std::vector<MeshRecord> moved;
    for (uint32_t idx : order)
    {
        const MeshRecord &o = blocks[idx];
        MeshRecord r = o;
        r.vBase = (uint32_t) (nVertices.used / 3);
        r.tBase = nTriangles.used / 3;
        r.eBase = (uint32_t) nKeys.used;
        const uint64_t ne = o.nv - o.nInternal;
        if (o.nv > 0)
            HIP_CHECK(hipMemcpyAsync(nVertices.ptr + nVertices.used, vertices.ptr + 3 * (uint64_t) o.vBase, 3 * (uint64_t) o.nv * sizeof(float),
                                     hipMemcpyDeviceToDevice, addStream));
        if (o.nt > 0)
        {
            HIP_CHECK(hipMemcpyAsync(nTriangles.ptr + nTriangles.used, triangles.ptr + 3 * o.tBase, 3 * o.nt * sizeof(uint32_t),
                                     hipMemcpyDeviceToDevice, addStream));
            hipLaunchKernelGGL(rebaseTrianglesKernel, dim3(divUp(3 * o.nt, 256)), dim3(256), 0, addStream,
                               nTriangles.ptr + nTriangles.used, 3 * o.nt, r.vBase - o.vBase);      /* modulo 2^32 */
        }
        if (ne > 0)
        {
            HIP_CHECK(hipMemcpyAsync(nKeys.ptr + nKeys.used, extKeys.ptr + o.eBase, ne * sizeof(uint64_t), hipMemcpyDeviceToDevice,
                                     addStream));
            hipLaunchKernelGGL(fillExternalsKernel, dim3(divUp(ne, 256)), dim3(256), 0, addStream, nGid.ptr + nGid.used,
                               nChunk.ptr + nChunk.used, ne, r.vBase + r.nInternal, (uint32_t) r.chunk);
        }
        nVertices.used += 3 * (uint64_t) o.nv;
        nTriangles.used += 3 * o.nt;
        nKeys.used += ne;
        nGid.used += ne;
        nChunk.used += ne;
        moved.push_back(r);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(addStream));
    std::swap(vertices.ptr, nVertices.ptr);
    std::swap(triangles.ptr, nTriangles.ptr);
    std::swap(extKeys.ptr, nKeys.ptr);
    std::swap(extGid.ptr, nGid.ptr);
    std::swap(extChunk.ptr, nChunk.ptr);
    blocks.swap(moved);
    return MLSGPU_OK;
}

/* What finalize, boundary and finalize_with start with: appends landed, blocks grouped by chunk, results emptied, slab and
 * outputs large enough and laid out.  `had`: what the slab holds of THESE arenas; a call that succeeds records its own. */
int mlsgpu_mesher::begin(SinkSizes &z, SinkScratch &L, SinkCache &had)
{
    PROPAGATE(drainPending());
    HIP_CHECK(hipSetDevice(ctx->device));
    dropResults();
    PROPAGATE(regroupByChunk());
    z = SinkSizes{vertices.used / 3, triangles.used / 3, extKeys.used, (uint32_t) blocks.size(), (uint32_t) chunkIds.size()};
    had = cache.matches(z.nv, z.nt, z.ne) ? cache : SinkCache();
    cache.drop();
    chunkVStart.assign(z.nc + 1, 0);
    chunkTStart.assign(z.nc + 1, 0);
    outChunks.clear();
    std::fill(stats, stats + 8, 0);
    if (z.empty())
        return MLSGPU_OK;
    const uint64_t slabBefore = slab.capacity();
    PROPAGATE(ensureSlab(scratchBytes(z)));
    if (slab.capacity() != slabBefore)
        had.drop();             /* (cannot happen for unchanged arenas; the cached analysis lived there) */
    PROPAGATE(ensureOutputs(z.nv, z.nt));
    Scratch S(slab, slab.capacity());
    PROPAGATE(L.lay(S, z));
    L.sortedInA = had.sortedInA;
    return MLSGPU_OK;
}

/* 1. every vertex its own representative, then the externals' from the sorted keys */
int mlsgpu_mesher::weld(SinkScratch &L, const SinkSizes &z)
{
    for (uint32_t *ids : {L.compRep, L.outRep, L.parent})       /* three launches */
        LAUNCH(ctx, "mesher.weld.time", iotaKernel, dim3(divUp(z.nv, 256)), B, ids, z.nv);
    HIP_CHECK(hipMemsetAsync(L.size, 0, z.nv * 4, ctx->stream));
    if (z.ne == 0)
        return MLSGPU_OK;
    SortResult<uint64_t> sorted = {nullptr, nullptr};
    HIP_CHECK(hipMemcpyAsync(L.keysA, extKeys.ptr, z.ne * 8, hipMemcpyDeviceToDevice, ctx->stream));
    PROPAGATE(radixSort<uint64_t>(ctx, "mesher.weld.time", L.keysA, L.slotsA, L.keysB, L.slotsB, z.ne, 64, true, L.hist,
                                  L.sortTileSums, &sorted));
    L.sortedInA = sorted.keys == L.keysA;
    LAUNCH(ctx, "mesher.weld.time", externalRepsKernel, dim3(divUp(z.ne, 256)), B, (const uint64_t *) sorted.keys,
           (const uint32_t *) sorted.vals, (const uint32_t *) extGid.ptr, (const uint32_t *) extChunk.ptr, z.ne, L.compRep, L.outRep);
    return MLSGPU_OK;
}

/* 2. union, roots, vertices per root */
int mlsgpu_mesher::components(const SinkScratch &L, const SinkSizes &z)
{
    /* measured in round 3 (ms per finalize, shortcut beyond 1 / 3 / 8 steps): shells cloud (17.8 M vertices) 13.3 / 12.8 /
     * 14.1, noise cloud (378 M) 113.9 / 103.9 / 96.3 */
    static const int forced = getenv("MLSGPU_HIP_UF_SHORTCUT") ? atoi(getenv("MLSGPU_HIP_UF_SHORTCUT")) : -1;
    const uint32_t unionShortcut = forced >= 0 ? (uint32_t) forced : (z.nv < (uint64_t(100) << 20) ? 3u : 8u);
    /* background (mlsgpu_hip_mesher_set_background): dynamic LDS the kernel never touches leaves it four workgroups per
     * CU.  The pass waits on L2 atomics, not on wave slots -- a surface-like mesh takes as long either way -- but at full
     * occupancy it slows the kernels of the job that is streaming in behind it. */
    const uint32_t ufPad = background && z.nv < (uint64_t(100) << 20) ? 40000u : 0u;        /* (a mesh of hundreds of millions
                                                                                             * of vertices does need the slots) */
    LAUNCH_LDS(ctx, "mesher.components.time", unionKernel, dim3(divUp(z.nt, 256)), B, ufPad, (const uint32_t *) triangles.ptr, z.nt,
               (const uint32_t *) L.compRep, L.parent, L.dFailed, unionShortcut);
    LAUNCH(ctx, "mesher.components.time", compressKernel, dim3(divUp(z.nv, 256)), B, L.parent, (const uint32_t *) L.compRep, z.nv, L.root);
    LAUNCH(ctx, "mesher.components.time", componentSizeKernel, dim3(divUp(divUp(z.nv, 64 * SIZE_SPAN), 4)), B,
           (const uint32_t *) L.compRep, (const uint32_t *) L.root, z.nv, L.size);
    return MLSGPU_OK;
}

/* 2b. several meshers, one job: the roots numbered densely in vertex order (the union-find hooks larger roots under smaller
 * ones, so a component's root is its smallest welded vertex whatever the schedule, and the numbering is reproducible) */
int mlsgpu_mesher::numberRoots(const SinkScratch &L, const SinkSizes &z, uint32_t *rootCount)
{
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "mesher.components.time", IsRootIn{L.compRep, L.root}, RootOut{L.rootId(), L.denseOf()},
                                       z.nv, 0u, L.rootTiles, L.dRootTotal)));
    HIP_CHECK(hipMemcpyAsync(rootCount, L.dRootTotal, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MLSGPU_OK;
}

/* vertices and triangles per root, in buffers of their own: representatives, roots and sizes stay intact for the verdict
 * pass (finalize_with) that follows an export; then the distinct keys with their roots */
int mlsgpu_mesher::exportBoundary(const SinkScratch &L, const SinkSizes &z, uint32_t rootCount)
{
    HIP_CHECK(hipMemsetAsync(L.tcount, 0, (size_t) rootCount * 4, ctx->stream));
    if (rootCount <= FEW_COMPONENTS)
        LAUNCH(ctx, "mesher.components.time", componentTrianglesFewKernel, dim3(divUp(divUp(z.nt, 64 * SIZE_SPAN), 4)), B,
               (const uint32_t *) triangles.ptr, (const uint32_t *) L.root, (const uint32_t *) L.denseOf(), z.nt, rootCount, L.tcount);
    else
        LAUNCH(ctx, "mesher.components.time", componentTrianglesKernel, dim3(divUp(divUp(z.nt, 64 * SIZE_SPAN), 4)), B,
               (const uint32_t *) triangles.ptr, (const uint32_t *) L.root, (const uint32_t *) L.denseOf(), z.nt, L.tcount);
    LAUNCH(ctx, "mesher.components.time", gatherSizesKernel, dim3(divUp(rootCount, 256)), B, (const uint32_t *) L.rootId(),
           (const uint32_t *) L.size, rootCount, L.vcount);
    std::vector<uint32_t> hv(rootCount), ht(rootCount);
    HIP_CHECK(hipMemcpyAsync(hv.data(), L.vcount, (size_t) rootCount * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(ht.data(), L.tcount, (size_t) rootCount * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (z.ne > 0)
    {
        uint32_t keyCount = 0;
        const KeyRootOut out{L.sortedKeys(), L.sortedSlots(), extGid.ptr, L.root, L.denseOf(), L.keyOut(), L.rootOut()};
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "mesher.weld.time", FirstOfRunIn{L.sortedKeys()}, out, z.ne, 0u, L.keyTiles, L.dKeyTotal)));
        HIP_CHECK(hipMemcpyAsync(&keyCount, L.dKeyTotal, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        PROPAGATE(bKeys.resize(keyCount));
        PROPAGATE(bKeyRoot.resize(keyCount));
        HIP_CHECK(hipMemcpyAsync(bKeys.data(), L.keyOut(), (size_t) keyCount * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(bKeyRoot.data(), L.rootOut(), (size_t) keyCount * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    bRootVertices.assign(hv.begin(), hv.end());
    bRootTriangles.assign(ht.begin(), ht.end());
    return MLSGPU_OK;
}

/* the caller's verdict per dense root (the numbering of the last export) over the component sizes: all or nothing */
int mlsgpu_mesher::applyVerdict(const SinkScratch &L, uint32_t rootCount, const uint8_t *keepRoots, uint64_t numRoots)
{
    if (numRoots != rootCount || !analyzed || bRootVertices.size() != rootCount)
        return setError(MLSGPU_ERR_LENGTH, "mesher: %llu verdicts for %u components (call boundary first, no add in between)",
                        (unsigned long long) numRoots, rootCount);
    HIP_CHECK(hipMemcpyAsync(L.dKeep, keepRoots, rootCount, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, "mesher.components.time", applyVerdictKernel, dim3(divUp(rootCount, 256)), dim3(256), (const uint32_t *) L.rootId(),
           (const uint8_t *) L.dKeep, rootCount, L.size);
    return MLSGPU_OK;
}

/* 3. the prune threshold (src/mesher.cpp:498-527): a component stays with at least max(minSize, uint64(welded vertices *
 * fraction)) vertices.  4. the output: two scans compact the kept vertices and triangles. */
int mlsgpu_mesher::writeOutput(const SinkScratch &L, const SinkSizes &z, double fraction, uint64_t minSize)
{
    const auto [nv, nt, ne, nb, nc] = z;
    HIP_CHECK(hipMemsetAsync(L.dStats, 0, 32, ctx->stream));
    const dim3 statsGrid((uint32_t) std::min<uint64_t>(divUp(nv, 256), 8192));
    LAUNCH(ctx, "mesher.components.time", componentStatsKernel, statsGrid, B, (const uint32_t *) L.compRep,
           (const uint32_t *) L.root, (const uint32_t *) L.size, nv, (uint64_t) 0, L.dStats, 0);
    unsigned long long hStats[4];
    HIP_CHECK(hipMemcpyAsync(hStats, L.dStats, 8, hipMemcpyDeviceToHost, ctx->stream));
    PROPAGATE(checkUnion(L));
    const uint64_t totalVertices = hStats[0];
    const uint64_t threshold = std::max(minSize, (uint64_t) ((double) totalVertices * fraction));
    LAUNCH(ctx, "mesher.components.time", componentStatsKernel, statsGrid, B, (const uint32_t *) L.compRep,
           (const uint32_t *) L.root, (const uint32_t *) L.size, nv, threshold, L.dStats, 1);

    std::vector<uint64_t> tBase(nb + 1), chunkFirstV(nc + 1), chunkFirstT(nc + 1);
    std::vector<uint32_t> vBase(nb + 1), chunkOf(nb);
    for (uint32_t b = 0; b < nb; b++)
    {
        tBase[b] = blocks[b].tBase;
        vBase[b] = blocks[b].vBase;
        chunkOf[b] = (uint32_t) blocks[b].chunk;
    }
    tBase[nb] = nt;
    vBase[nb] = (uint32_t) nv;
    for (uint32_t c = 0, b = 0; c <= nc; c++)
    {
        while (b < nb && chunkOf[b] < c)
            b++;
        chunkFirstV[c] = b < nb ? vBase[b] : nv;
        chunkFirstT[c] = b < nb ? tBase[b] : nt;
    }
    HIP_CHECK(hipMemcpyAsync(L.dTBase, tBase.data(), (nb + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(L.dVBase, vBase.data(), (nb + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(L.dChunkOf, chunkOf.data(), nb * 4, hipMemcpyHostToDevice, ctx->stream));

    /* vertices: the scan's size is not known before it ran; the output is sized for every vertex and trimmed by count */
    const KeepVertexIn keepV{L.outRep, L.root, L.size, threshold};
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "mesher.output.time", keepV, VertexOut{vertices.ptr, outVertices, L.vIndex},
                                       nv, 0u, L.tileSums, L.dTotals)));
    HIP_CHECK(hipMemcpyAsync(L.dAt, chunkFirstV.data(), (nc + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, "mesher.output.time", gatherU32Kernel, dim3(divUp(nc + 1, 256)), B, (const uint32_t *) L.vIndex,
           (const uint64_t *) L.dAt, nc + 1, nv, 0u, L.dChunkVStart);
    /* the entry for "one past the last vertex" is the scan total */
    std::vector<uint32_t> hV(nc + 1), hT(nc + 1);
    uint32_t totals[2] = {0, 0};
    HIP_CHECK(hipMemcpyAsync(hV.data(), L.dChunkVStart, (nc + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(&totals[0], L.dTotals, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (uint32_t c = 0; c <= nc; c++)
        if (chunkFirstV[c] >= nv)
            hV[c] = totals[0];
    HIP_CHECK(hipMemcpyAsync(L.dChunkVStart, hV.data(), (nc + 1) * 4, hipMemcpyHostToDevice, ctx->stream));

    /* triangles */
    const BlockTable T{L.dTBase, L.dVBase, L.dChunkOf, L.dChunkVStart, nb};
    const KeepTriangleIn keepT{triangles.ptr, L.root, L.size, threshold};
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "mesher.output.time", keepT,
                                       TriangleOutIdx{TriangleOut{triangles.ptr, L.outRep, L.vIndex, T, outTriangles}, L.tIndex},
                                       nt, 0u, L.tileSums, L.dTotals + 1)));
    HIP_CHECK(hipMemcpyAsync(L.dAt, chunkFirstT.data(), (nc + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, "mesher.output.time", gatherU32Kernel, dim3(divUp(nc + 1, 256)), B, (const uint32_t *) L.tIndex,
           (const uint64_t *) L.dAt, nc + 1, nt, 0u, L.dChunkTStart);
    HIP_CHECK(hipMemcpyAsync(hT.data(), L.dChunkTStart, (nc + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(&totals[1], L.dTotals + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(hStats, L.dStats, 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (uint32_t c = 0; c <= nc; c++)
    {
        chunkVStart[c] = hV[c];
        chunkTStart[c] = chunkFirstT[c] >= nt ? totals[1] : hT[c];
    }
    for (uint32_t c = 0; c < nc; c++)
        if (chunkTStart[c + 1] > chunkTStart[c])      /* no output for a chunk without triangles, :820 */
            outChunks.push_back(c);
    const uint64_t all[8] = {totalVertices, threshold, hStats[1], hStats[2], hStats[3], totals[1], nv, nt};
    std::copy(all, all + 8, stats);
    return MLSGPU_OK;
}

/* MesherBase::write's finalisation (src/mesher.cpp:763-852) up to the point where files are written */
MLSGPU_API int mlsgpu_hip_mesher_finalize(mlsgpu_mesher *m, uint32_t *numChunks)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    SinkSizes z;
    SinkScratch L;
    SinkCache had;
    PROPAGATE(m->begin(z, L, had));
    if (z.empty())
        return m->finish(numChunks);
    PROPAGATE(m->analyse(L, z, false));
    PROPAGATE(m->writeOutput(L, z, m->pruneThreshold, 0));
    m->cache = SinkCache{SinkCache::AfterFinalize, L.sortedInA, z.nv, z.nt, z.ne, 0};
    return m->finish(numChunks);
}

MLSGPU_API int mlsgpu_hip_mesher_chunk(mlsgpu_mesher *m, uint32_t i, uint64_t *chunkId, uint64_t *numVertices,
                                       uint64_t *numTriangles, const float **dVertices, const uint32_t **dTriangles)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(m->finalized && i < m->outChunks.size(), MLSGPU_ERR_INVALID);
    const mlsgpu_mesher::Span s = m->span(m->outChunks[i]);
    if (chunkId) *chunkId = m->chunkIds[m->outChunks[i]];
    if (numVertices) *numVertices = s.nv;
    if (numTriangles) *numTriangles = s.nt;
    if (dVertices) *dVertices = m->outVertices + 3 * s.v0;
    if (dTriangles) *dTriangles = m->outTriangles + 3 * s.t0;
    return MLSGPU_OK;
}

/* the topology report (topology.hip) of output chunk i, where it lies */
MLSGPU_API int mlsgpu_hip_mesher_chunk_topology(mlsgpu_mesher *m, uint32_t i, mlsgpu_topology *out)
{
    REQUIRE(m != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized && i < m->outChunks.size(), MLSGPU_ERR_INVALID);
    const mlsgpu_mesher::Span s = m->span(m->outChunks[i]);
    return mlsgpu_hip_mesh_topology(m->ctx, m->outTriangles + 3 * s.t0, s.nt, s.nv, out);
}

/* ---- the stages that work on the finished chunks: their statistics' folds, then the three routes a stage takes ---- */

using Span = mlsgpu_mesher::Span;

/* accumulate(total, one, first): the statistics of one chunk join the sink's; `first` says that no chunk was folded before.
 * The counts add up.  What does not start at zero (converged, the smallest lengths, smooth's passes) is preset by the entry
 * point, where it can be seen. */

/* the largest exponent among the chunks that have one: `first` among those */
static void foldExponent(int64_t &total, int64_t one, bool first) { total = first ? one : std::max(total, one); }

/* the six counts that mlsgpu_simplify_stats and mlsgpu_simplify_quadric_stats share */
template<typename Stats>
static void addSimplifyCounts(Stats &total, const Stats &one)
{
    total.inVertices += one.inVertices;
    total.inTriangles += one.inTriangles;
    total.outVertices += one.outVertices;
    total.outTriangles += one.outTriangles;
    total.collapsedTriangles += one.collapsedTriangles;
    total.duplicateTriangles += one.duplicateTriangles;
}

static void accumulate(mlsgpu_simplify_stats &total, const mlsgpu_simplify_stats &one, bool) { addSimplifyCounts(total, one); }

static void accumulate(mlsgpu_simplify_quadric_stats &total, const mlsgpu_simplify_quadric_stats &one, bool)
{
    /* a chunk has a scale where M != 0: where it solved or escaped */
    const bool scaledBefore = total.solvedVertices + total.escapedVertices > 0;
    addSimplifyCounts(total, one);
    total.solvedVertices += one.solvedVertices;
    total.flatVertices += one.flatVertices;
    total.escapedVertices += one.escapedVertices;
    if (one.solvedVertices + one.escapedVertices > 0)
        foldExponent(total.scaleExponent, one.scaleExponent, !scaledBefore);
}

static void accumulate(mlsgpu_smooth_stats &total, const mlsgpu_smooth_stats &one, bool first)
{
    total.numVertices += one.numVertices;
    total.numTriangles += one.numTriangles;
    total.outOfRangeTriangles += one.outOfRangeTriangles;
    total.degenerateTriangles += one.degenerateTriangles;
    total.numEdges += one.numEdges;
    total.boundaryEdges += one.boundaryEdges;
    total.boundaryVertices += one.boundaryVertices;
    total.isolatedVertices += one.isolatedVertices;
    total.passes = one.passes;          /* the last chunk's: the same for all of them */
    foldExponent(total.scaleExponent, one.scaleExponent, first);
    total.maxMove = std::max(total.maxMove, one.maxMove);
    total.maxCoordinate = std::max(total.maxCoordinate, one.maxCoordinate);
}

/* what mlsgpu_flip_stats, mlsgpu_collapse_stats and mlsgpu_split_stats share: the input's counts, the rounds (the most of any chunk, converged if
 * all did) and the quality report, whose minima have no neutral start value */
template<typename Stats>
static void addEdgeRounds(Stats &total, const Stats &one, bool first)
{
    total.numVertices += one.numVertices;
    total.numTriangles += one.numTriangles;
    total.outOfRangeTriangles += one.outOfRangeTriangles;
    total.degenerateTriangles += one.degenerateTriangles;
    total.numEdges += one.numEdges;
    total.interiorEdges += one.interiorEdges;
    total.rounds = std::max(total.rounds, one.rounds);
    total.converged &= one.converged;
    total.blockedAfter += one.blockedAfter;
    total.minQualityBefore = first ? one.minQualityBefore : std::min(total.minQualityBefore, one.minQualityBefore);
    total.minQualityAfter = first ? one.minQualityAfter : std::min(total.minQualityAfter, one.minQualityAfter);
    for (int k = 0; k < 16; k++)
    {
        total.qualityBefore[k] += one.qualityBefore[k];
        total.qualityAfter[k] += one.qualityAfter[k];
    }
}

static void accumulate(mlsgpu_flip_stats &total, const mlsgpu_flip_stats &one, bool first)
{
    addEdgeRounds(total, one, first);
    total.flips += one.flips;
    total.nonDelaunayBefore += one.nonDelaunayBefore;
    total.nonDelaunayAfter += one.nonDelaunayAfter;
}

static void accumulate(mlsgpu_collapse_stats &total, const mlsgpu_collapse_stats &one, bool first)
{
    addEdgeRounds(total, one, first);
    total.fixedVertices += one.fixedVertices;
    total.collapses += one.collapses;
    total.shortBefore += one.shortBefore;
    total.shortAfter += one.shortAfter;
    total.unusedVertices += one.unusedVertices;
    total.outVertices += one.outVertices;
    total.outTriangles += one.outTriangles;
    total.minLengthSqBefore = std::min(total.minLengthSqBefore, one.minLengthSqBefore);
    total.minLengthSqAfter = std::min(total.minLengthSqAfter, one.minLengthSqAfter);
}

static void accumulate(mlsgpu_split_stats &total, const mlsgpu_split_stats &one, bool first)
{
    addEdgeRounds(total, one, first);
    total.boundaryEdges += one.boundaryEdges;
    total.splits += one.splits;
    total.boundarySplits += one.boundarySplits;
    total.limited |= one.limited;
    total.longBefore += one.longBefore;
    total.longAfter += one.longAfter;
    total.outVertices += one.outVertices;
    total.outTriangles += one.outTriangles;
    total.maxLengthSqBefore = std::max(total.maxLengthSqBefore, one.maxLengthSqBefore);
    total.maxLengthSqAfter = std::max(total.maxLengthSqAfter, one.maxLengthSqAfter);
}

static void accumulate(mlsgpu_fill_stats &total, const mlsgpu_fill_stats &one, bool first)
{
    total.numVertices += one.numVertices;
    total.numTriangles += one.numTriangles;
    total.outOfRangeTriangles += one.outOfRangeTriangles;
    total.degenerateTriangles += one.degenerateTriangles;
    total.boundaryEdges += one.boundaryEdges;
    total.irregularEdges += one.irregularEdges;
    total.loops += one.loops;
    total.filledLoops += one.filledLoops;
    total.longLoops += one.longLoops;
    total.pinnedLoops += one.pinnedLoops;
    total.filledEdges += one.filledEdges;
    total.longestLoop = std::max(total.longestLoop, one.longestLoop);
    total.outVertices += one.outVertices;
    total.outTriangles += one.outTriangles;
    foldExponent(total.scaleExponent, one.scaleExponent, first);
}

static void accumulate(mlsgpu_repair_stats &total, const mlsgpu_repair_stats &one, bool)
{
    total.numVertices += one.numVertices;
    total.numTriangles += one.numTriangles;
    total.outOfRangeTriangles += one.outOfRangeTriangles;
    total.degenerateTriangles += one.degenerateTriangles;
    total.repeatedSides += one.repeatedSides;
    total.droppedTriangles += one.droppedTriangles;
    total.unusedVertices += one.unusedVertices;
    total.splitVertices += one.splitVertices;
    total.addedVertices += one.addedVertices;
    total.outVertices += one.outVertices;
    total.outTriangles += one.outTriangles;
}

/* *total += the report of dense chunk c: the counts add, the maximum and the lowest (chunk, point) that attains it are kept.
 * The chunks come in ascending order, so a later chunk takes the maximum over only by exceeding it. */
static void addDeviation(mlsgpu_deviation *total, const mlsgpu_deviation &one, uint64_t c)
{
    total->numPoints += one.numPoints;
    total->numVertices += one.numVertices;
    total->numTriangles += one.numTriangles;
    total->outOfRangeTriangles += one.outOfRangeTriangles;
    total->degenerateTriangles += one.degenerateTriangles;
    total->beyond += one.beyond;
    for (int k = 0; k < 16; k++)
        total->histogram[k] += one.histogram[k];
    total->sumQ += one.sumQ;
    if (one.numPoints > 0)
        total->scaleExponent = one.scaleExponent;       /* D is the same for every chunk, hence e */
    if (one.within > 0 && (total->within == 0 || one.maxDistance2 > total->maxDistance2))
    {
        total->maxDistance2 = one.maxDistance2;
        total->farthestChunk = c;
        total->farthestPoint = one.farthestPoint;
    }
    total->within += one.within;
}

/* The three routes.  Each is for the holder of the lock of a finalized sink, after the entry point has checked the stage's
 * parameters (a refused parameter costs no results) and preset *total; each hands every dense chunk that has triangles to
 * `stage`, which calls the mesh function on the chunk where it lies, and folds what it reports into *total.  A chunk without
 * triangles has no output (finalize) and is skipped.  The two routes that write the chunks anew (to the front, into a new
 * generation) keep nothing of it; the in-place route leaves it alone, so vertices that finalize kept in it (welded to another
 * chunk's component) stay until a stage of the other two routes runs.  Until then the seam mask and the deviation report,
 * which walk the dense chunks, see them. */

/* To the front (simplify): stage(chunk, outVertices, outTriangles, &one) writes into buffers of the largest chunk's size, and from
 * there the result goes to the front of the output arrays: it is never larger than its chunk, so chunk c's lands at or before
 * where chunk c began and never on a chunk that is still to be read.  A failure after the first chunk costs the results. */
template<typename Stats, typename Stage>
static int simplifyChunks(mlsgpu_mesher *m, Stats *total, Stage stage)
{
    mlsgpu_ctx *const ctx = m->ctx;
    HIP_CHECK(hipSetDevice(ctx->device));
    m->dropNormals();           /* the chunks change and move */
    const size_t nc = m->chunkVStart.size() - 1;        /* finalize sized the tables: [chunks + 1] */
    uint64_t maxV = 0, maxT = 0;
    for (size_t c = 0; c < nc; c++)
    {
        maxV = std::max(maxV, m->span(c).nv);
        maxT = std::max(maxT, m->span(c).nt);
    }
    DeviceArray<float> tmpV;
    DeviceArray<uint32_t> tmpT;
    PROPAGATE(tmpV.alloc(3 * maxV));
    PROPAGATE(tmpT.alloc(3 * maxT));
    uint64_t vAt = 0, tAt = 0;
    for (size_t c = 0; c < nc; c++)
    {
        const Span s = m->span(c);
        Stats one;
        std::memset(&one, 0, sizeof(one));
        int rc = s.nt > 0 ? stage(s, tmpV.get(), tmpT.get(), &one) : MLSGPU_OK;
        if (rc == MLSGPU_OK && one.outVertices > 0
            && hipMemcpyAsync(m->outVertices + 3 * vAt, tmpV, one.outVertices * 12, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
            rc = setError(MLSGPU_ERR_HIP, "mesher simplify: the copy of a chunk's vertices failed");
        if (rc == MLSGPU_OK && one.outTriangles > 0
            && hipMemcpyAsync(m->outTriangles + 3 * tAt, tmpT, one.outTriangles * 12, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess)
            rc = setError(MLSGPU_ERR_HIP, "mesher simplify: the copy of a chunk's triangles failed");
        if (rc != MLSGPU_OK)
        {
            if (c > 0)
                m->dropResults();       /* earlier chunks have moved: the chunk table no longer describes the arrays */
            return rc;
        }
        m->chunkVStart[c] = vAt;
        m->chunkTStart[c] = tAt;
        vAt += one.outVertices;
        tAt += one.outTriangles;
        accumulate(*total, one, c == 0);
    }
    m->chunkVStart[nc] = vAt;
    m->chunkTStart[nc] = tAt;
    HIP_CHECK(hipStreamSynchronize(ctx->stream));       /* the temporaries go with the call */
    return MLSGPU_OK;
}

/* In place (smooth, flip): stage(chunk, &one) writes over the chunk; a chunk without triangles stays as it is, vertices
 * included.  A failure costs the results: earlier chunks are changed already, and the one that failed holds what it reached. */
template<typename Stats, typename Stage>
static int stageInPlace(mlsgpu_mesher *m, Stats *total, Stage stage)
{
    m->dropNormals();           /* the positions or the triangles change */
    const size_t nc = m->chunkVStart.size() - 1;        /* finalize sized the tables: [chunks + 1] */
    bool first = true;
    for (size_t c = 0; c < nc; c++)
    {
        const Span s = m->span(c);
        if (s.nt == 0)
            continue;
        Stats one;
        const int rc = stage(s, &one);
        if (rc != MLSGPU_OK)
        {
            m->dropResults();
            return rc;
        }
        accumulate(*total, one, first);
        first = false;
    }
    return MLSGPU_OK;
}

/* Into a new generation (fill, repair, collapse, split): the chunks change size and may grow, so they cannot stay where they lie.
 * stage(chunk, outVertices, vertexCapacity, outTriangles, triangleCapacity, &one) is called twice per chunk: without room
 * at all it stops at its capacity check with the sizes in `one` (MLSGPU_ERR_LENGTH; MLSGPU_OK where it keeps nothing, and is
 * done), then it writes into new arrays, behind the chunk before.  Nothing of the sink changes before the last chunk is done:
 * a failure leaves the results as they were. */
template<typename Stats, typename Stage>
static int stageIntoNewGeneration(mlsgpu_mesher *m, Stats *total, Stage stage)
{
    HIP_CHECK(hipSetDevice(m->ctx->device));
    const size_t nc = m->chunkVStart.size() - 1;        /* finalize sized the tables: [chunks + 1] */
    std::vector<Stats> one(nc);
    std::vector<uint64_t> vStart(nc + 1, 0), tStart(nc + 1, 0);
    for (size_t c = 0; c < nc; c++)
    {
        std::memset(&one[c], 0, sizeof(one[c]));
        if (m->span(c).nt > 0)
        {
            const int rc = stage(m->span(c), nullptr, 0, nullptr, 0, &one[c]);
            if (rc != MLSGPU_ERR_LENGTH && rc != MLSGPU_OK)
                return rc;
        }
        vStart[c + 1] = vStart[c] + one[c].outVertices;
        tStart[c + 1] = tStart[c] + one[c].outTriangles;
    }
    DeviceArray<float> newVertices;
    DeviceArray<uint32_t> newTriangles;
    PROPAGATE(newVertices.alloc(std::max<uint64_t>(3 * vStart[nc], 1)));
    PROPAGATE(newTriangles.alloc(std::max<uint64_t>(3 * tStart[nc], 1)));
    bool first = true;
    for (size_t c = 0; c < nc; c++)
    {
        if (m->span(c).nt == 0)
            continue;
        if (one[c].outTriangles > 0)
            PROPAGATE(stage(m->span(c), newVertices + 3 * vStart[c], one[c].outVertices, newTriangles + 3 * tStart[c], one[c].outTriangles,
                            &one[c]));
        accumulate(*total, one[c], first);
        first = false;
    }
    /* the new generation takes the old one's place (which goes with this call) */
    m->outVertices = std::move(newVertices);
    m->outTriangles = std::move(newTriangles);
    m->chunkVStart = vStart;
    m->chunkTStart = tStart;
    m->dropNormals();           /* the chunks have changed and moved */
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesher_simplify(mlsgpu_mesher *m, const float origin[3], float cellSize, mlsgpu_simplify_stats *stats)
{
    REQUIRE(m != nullptr && origin != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    return simplifyChunks(m, stats, [&](const Span &s, float *outV, uint32_t *outT, mlsgpu_simplify_stats *one) {
        return mlsgpu_hip_mesh_simplify(m->ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, origin, cellSize, outV,
                                        outT, one);
    });
}

MLSGPU_API int mlsgpu_hip_mesher_simplify_quadric(mlsgpu_mesher *m, const float origin[3], float cellSize,
                                                  mlsgpu_simplify_quadric_stats *stats)
{
    REQUIRE(m != nullptr && origin != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    return simplifyChunks(m, stats, [&](const Span &s, float *outV, uint32_t *outT, mlsgpu_simplify_quadric_stats *one) {
        return mlsgpu_hip_mesh_simplify_quadric(m->ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, origin, cellSize,
                                                outV, outT, one);
    });
}

/* Every output chunk through mlsgpu_hip_mesh_smooth (smooth.hip), in place: only the positions change. */
MLSGPU_API int mlsgpu_hip_mesher_smooth(mlsgpu_mesher *m, uint32_t iterations, float lambda, float mu, uint32_t boundary,
                                        mlsgpu_smooth_stats *stats)
{
    REQUIRE(m != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    /* mlsgpu_hip_mesh_smooth's own checks, here so that a refused parameter costs no results */
    REQUIRE(std::isfinite(lambda) && lambda > 0.0f && lambda <= 1.0f && std::isfinite(mu) && mu >= -1.0f && mu <= 0.0f, MLSGPU_ERR_INVALID);
    REQUIRE(boundary == MLSGPU_SMOOTH_BOUNDARY_FIXED || boundary == MLSGPU_SMOOTH_BOUNDARY_CURVE, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->passes = (uint64_t) iterations * (mu != 0.0f ? 2 : 1);
    return stageInPlace(m, stats, [&](const Span &s, mlsgpu_smooth_stats *one) {
        return mlsgpu_hip_mesh_smooth(m->ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, iterations, lambda, mu,
                                      boundary, m->outVertices + 3 * s.v0, one);
    });
}

/* Every output chunk through mlsgpu_hip_mesh_flip_edges (flip.hip), in place: only the triangles change. */
MLSGPU_API int mlsgpu_hip_mesher_flip_edges(mlsgpu_mesher *m, uint32_t maxRounds, double minGain, double minCos, mlsgpu_flip_stats *stats)
{
    REQUIRE(m != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    /* mlsgpu_hip_mesh_flip_edges's own checks, here so that a refused parameter costs no results */
    REQUIRE(std::isfinite(minGain) && minGain >= 0.0 && minCos >= -1.0 && minCos <= 1.0, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->converged = maxRounds > 0 ? 1 : 0;       /* the AND over the chunks starts where a mesh without triangles ends */
    return stageInPlace(m, stats, [&](const Span &s, mlsgpu_flip_stats *one) {
        return mlsgpu_hip_mesh_flip_edges(m->ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, maxRounds, minGain,
                                          minCos, m->outTriangles + 3 * s.t0, one);
    });
}

/* Every output chunk that has triangles through mlsgpu_hip_mesh_fill_holes (fill.hip), into a new generation: the chunks grow. */
MLSGPU_API int mlsgpu_hip_mesher_fill_holes(mlsgpu_mesher *m, uint32_t maxEdges, mlsgpu_fill_stats *stats)
{
    REQUIRE(m != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    /* mlsgpu_hip_mesh_fill_holes's own check, here so that a refused parameter does no work */
    REQUIRE(maxEdges >= 3 && maxEdges <= MLSGPU_FILL_MAX_EDGES, MLSGPU_ERR_INVALID);
    mlsgpu_ctx *const ctx = m->ctx;
    HIP_CHECK(hipSetDevice(ctx->device));
    std::memset(stats, 0, sizeof(*stats));
    /* the seams: with several chunks, a vertex that another chunk has too is pinned */
    DeviceArray<uint8_t> pinned;
    if (m->outChunks.size() > 1)
    {
        const size_t nc = m->chunkVStart.size() - 1;    /* finalize sized the tables: [chunks + 1] */
        PROPAGATE(pinned.alloc(m->chunkVStart[nc]));
        PROPAGATE(seamMask(ctx, m->outVertices, m->chunkVStart[nc], m->chunkVStart.data(), (uint32_t) nc, pinned));
    }
    return stageIntoNewGeneration(m, stats, [&](const Span &s, float *outV, uint64_t capV, uint32_t *outT, uint64_t capT,
                                                mlsgpu_fill_stats *one) {
        return mlsgpu_hip_mesh_fill_holes(ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, maxEdges,
                                          pinned.get() != nullptr ? pinned + s.v0 : nullptr, outV, capV, outT, capT, one);
    });
}

/* Every output chunk that has triangles through mlsgpu_hip_mesh_repair (repair.hip), into a new generation: a chunk can grow
 * in vertices. */
MLSGPU_API int mlsgpu_hip_mesher_repair(mlsgpu_mesher *m, uint32_t flags, mlsgpu_repair_stats *stats)
{
    REQUIRE(m != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    /* mlsgpu_hip_mesh_repair's own check, here so that a refused parameter does no work */
    REQUIRE((flags & ~(uint32_t) MLSGPU_REPAIR_SPLIT_PINCHES) == 0, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    return stageIntoNewGeneration(m, stats, [&](const Span &s, float *outV, uint64_t capV, uint32_t *outT, uint64_t capT,
                                                mlsgpu_repair_stats *one) {
        return mlsgpu_hip_mesh_repair(m->ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, flags, outV, capV, outT,
                                      capT, nullptr, one);
    });
}

/* Every output chunk that has triangles through mlsgpu_hip_mesh_collapse_edges (collapse.hip), into a new generation. */
MLSGPU_API int mlsgpu_hip_mesher_collapse_edges(mlsgpu_mesher *m, uint32_t maxRounds, double maxLength, double minCos,
                                                mlsgpu_collapse_stats *stats)
{
    REQUIRE(m != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    /* mlsgpu_hip_mesh_collapse_edges's own checks, here so that a refused parameter does no work */
    REQUIRE(std::isfinite(maxLength) && maxLength >= 0.0 && minCos >= 0.0 && minCos <= 1.0, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->converged = maxRounds > 0 ? 1 : 0;       /* the AND over the chunks starts where a mesh without triangles ends */
    stats->minLengthSqBefore = stats->minLengthSqAfter = INFINITY;
    return stageIntoNewGeneration(m, stats, [&](const Span &s, float *outV, uint64_t capV, uint32_t *outT, uint64_t capT,
                                                mlsgpu_collapse_stats *one) {
        return mlsgpu_hip_mesh_collapse_edges(m->ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, maxRounds,
                                              maxLength, minCos, outV, capV, outT, capT, nullptr, one);
    });
}

/* Every output chunk that has triangles through mlsgpu_hip_mesh_split_edges (split.hip), into a new generation: the chunks
 * grow.  The seams are pinned as for the hole filling. */
MLSGPU_API int mlsgpu_hip_mesher_split_edges(mlsgpu_mesher *m, uint32_t maxRounds, double maxLength, uint32_t maxGrowth,
                                             mlsgpu_split_stats *stats)
{
    REQUIRE(m != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    /* mlsgpu_hip_mesh_split_edges's own check, here so that a refused parameter does no work */
    REQUIRE(std::isfinite(maxLength) && maxLength > 0.0, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    mlsgpu_ctx *const ctx = m->ctx;
    HIP_CHECK(hipSetDevice(ctx->device));
    std::memset(stats, 0, sizeof(*stats));
    stats->converged = maxRounds > 0 ? 1 : 0;       /* the AND over the chunks starts where a mesh without triangles ends */
    /* the seams: with several chunks, a vertex that another chunk has too is pinned */
    DeviceArray<uint8_t> pinned;
    if (m->outChunks.size() > 1)
    {
        const size_t nc = m->chunkVStart.size() - 1;    /* finalize sized the tables: [chunks + 1] */
        PROPAGATE(pinned.alloc(m->chunkVStart[nc]));
        PROPAGATE(seamMask(ctx, m->outVertices, m->chunkVStart[nc], m->chunkVStart.data(), (uint32_t) nc, pinned));
    }
    return stageIntoNewGeneration(m, stats, [&](const Span &s, float *outV, uint64_t capV, uint32_t *outT, uint64_t capT,
                                                mlsgpu_split_stats *one) {
        return mlsgpu_hip_mesh_split_edges(ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, maxRounds, maxLength,
                                           (uint64_t) maxGrowth * s.nt, pinned.get() != nullptr ? pinned + s.v0 : nullptr, outV, capV,
                                           outT, capT, nullptr, one);
    });
}

/* ---- the deviation report of the sink against a kept copy of itself (deviation.hip) ---- */

MLSGPU_API int mlsgpu_hip_mesher_keep_reference(mlsgpu_mesher *m)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    mlsgpu_ctx *const ctx = m->ctx;
    HIP_CHECK(hipSetDevice(ctx->device));
    m->dropReference();
    const uint64_t nv = m->chunkVStart.back(), nt = m->chunkTStart.back();
    PROPAGATE(m->refVertices.alloc(3 * nv));
    PROPAGATE(m->refTriangles.alloc(3 * nt));
    if (nv > 0)
        HIP_CHECK(hipMemcpyAsync(m->refVertices, m->outVertices, nv * 12, hipMemcpyDeviceToDevice, ctx->stream));
    if (nt > 0)
        HIP_CHECK(hipMemcpyAsync(m->refTriangles, m->outTriangles, nt * 12, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    m->refVStart = m->chunkVStart;
    m->refTStart = m->chunkTStart;
    m->referenceKept = true;
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesher_drop_reference(mlsgpu_mesher *m)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    m->dropReference();
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesher_deviation(mlsgpu_mesher *m, float maxDistance, mlsgpu_deviation *moved, mlsgpu_deviation *lost)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized && m->referenceKept && m->refVStart.size() == m->chunkVStart.size(), MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(maxDistance) && maxDistance > 0.0f, MLSGPU_ERR_INVALID);
    mlsgpu_ctx *const ctx = m->ctx;
    const size_t nc = m->chunkVStart.size() - 1;        /* finalize sized the tables: [chunks + 1] */
    mlsgpu_deviation *const totals[2] = {moved, lost};
    for (mlsgpu_deviation *total : totals)
        if (total != nullptr)
        {
            std::memset(total, 0, sizeof(*total));
            total->farthestPoint = UINT64_MAX;
            total->limit2 = (double) maxDistance * (double) maxDistance;
        }
    for (size_t c = 0; c < nc; c++)
    {
        const mlsgpu_mesher::Span now = m->span(c);
        const mlsgpu_mesher::Span kept = {m->refVStart[c], m->refTStart[c], m->refVStart[c + 1] - m->refVStart[c],
                                          m->refTStart[c + 1] - m->refTStart[c]};
        mlsgpu_deviation one;
        if (moved != nullptr)
        {
            PROPAGATE(mlsgpu_hip_mesh_deviation(ctx, m->outVertices + 3 * now.v0, now.nv, m->refVertices + 3 * kept.v0, kept.nv,
                                                m->refTriangles + 3 * kept.t0, kept.nt, maxDistance, nullptr, nullptr, &one));
            addDeviation(moved, one, c);
        }
        if (lost != nullptr)
        {
            PROPAGATE(mlsgpu_hip_mesh_deviation(ctx, m->refVertices + 3 * kept.v0, kept.nv, m->outVertices + 3 * now.v0, now.nv,
                                                m->outTriangles + 3 * now.t0, now.nt, maxDistance, nullptr, nullptr, &one));
            addDeviation(lost, one, c);
        }
    }
    return MLSGPU_OK;
}

/* The self-intersection report (intersect.hip) of every dense chunk, added up: the chunks come in ascending order, so the
 * first one with a crossing names the lowest pair and a later one takes the maximum over only by exceeding it. */
MLSGPU_API int mlsgpu_hip_mesher_self_intersections(mlsgpu_mesher *m, mlsgpu_self_intersections *out)
{
    REQUIRE(m != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized, MLSGPU_ERR_INVALID);
    mlsgpu_ctx *const ctx = m->ctx;
    const size_t nc = m->chunkVStart.size() - 1;        /* finalize sized the tables: [chunks + 1] */
    std::memset(out, 0, sizeof(*out));
    out->lowestA = out->lowestB = out->maxPartnersTriangle = UINT64_MAX;
    for (size_t c = 0; c < nc; c++)
    {
        const auto [v0, t0, nv, nt] = m->span(c);
        mlsgpu_self_intersections one;
        PROPAGATE(mlsgpu_hip_mesh_self_intersections(ctx, m->outVertices + 3 * v0, nv, m->outTriangles + 3 * t0, nt, nullptr, nullptr, 0,
                                                     &one));
        out->numVertices += one.numVertices;
        out->numTriangles += one.numTriangles;
        out->outOfRangeTriangles += one.outOfRangeTriangles;
        out->degenerateTriangles += one.degenerateTriangles;
        out->candidatePairs += one.candidatePairs;
        out->crossingPairs += one.crossingPairs;
        out->crossingTriangles += one.crossingTriangles;
        if (one.crossingPairs == 0)
            continue;
        if (out->crossingChunks++ == 0)
        {
            out->lowestChunk = c;
            out->lowestA = one.lowestA;
            out->lowestB = one.lowestB;
        }
        if (one.maxPartners > out->maxPartners)
        {
            out->maxPartners = one.maxPartners;
            out->maxPartnersTriangle = one.maxPartnersTriangle;
        }
    }
    return MLSGPU_OK;
}

/* Output chunk i encoded where it lies (compact.hip) and copied to the caller's host memory; only reads the sink. */
MLSGPU_API int mlsgpu_hip_mesher_chunk_compact(mlsgpu_mesher *m, uint32_t i, uint32_t vertexBits, void *hostBlob, uint64_t capacityBytes,
                                               mlsgpu_compact_stats *stats)
{
    REQUIRE(m != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized && i < m->outChunks.size(), MLSGPU_ERR_INVALID);
    const mlsgpu_mesher::Span s = m->span(m->outChunks[i]);
    return compactMesh(m->ctx, m->outVertices + 3 * s.v0, s.nv, m->outTriangles + 3 * s.t0, s.nt, vertexBits, nullptr, hostBlob,
                       capacityBytes, stats);
}

/* The normals (normals.hip) of dense chunk c of a finalized sink, computed where the chunk lies at the first request.  Under
 * the mutex. */
int mlsgpu_mesher::chunkNormals(uint32_t c, const float **dNormals, mlsgpu_normals_stats *out)
{
    const size_t nc = chunkVStart.size() - 1;
    const uint64_t total = chunkVStart[nc];
    HIP_CHECK(hipSetDevice(ctx->device));
    if (outNormals.get() == nullptr || outNormals.capacity() < 3 * total)
    {
        dropNormals();          /* growing discards what was computed */
        PROPAGATE(outNormals.reserve(std::max<uint64_t>(3 * total, 1)));
    }
    if (normalsReady.size() != nc)
    {
        normalsReady.assign(nc, 0);
        normalsOf.assign(nc, mlsgpu_normals_stats());
    }
    const Span s = span(c);
    if (!normalsReady[c])
    {
        PROPAGATE(mlsgpu_hip_mesh_normals(ctx, outVertices + 3 * s.v0, s.nv, outTriangles + 3 * s.t0, s.nt, outNormals + 3 * s.v0,
                                          &normalsOf[c]));
        normalsReady[c] = 1;
    }
    if (dNormals) *dNormals = outNormals + 3 * s.v0;
    if (out) *out = normalsOf[c];
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesher_chunk_normals(mlsgpu_mesher *m, uint32_t i, const float **dNormals, mlsgpu_normals_stats *stats)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized && i < m->outChunks.size(), MLSGPU_ERR_INVALID);
    return m->chunkNormals(m->outChunks[i], dNormals, stats);
}

MLSGPU_API int mlsgpu_hip_mesher_stats(mlsgpu_mesher *m, uint64_t out[8])
{
    REQUIRE(m != nullptr && out != nullptr && m->finalized, MLSGPU_ERR_INVALID);
    std::copy(m->stats, m->stats + 8, out);
    return MLSGPU_OK;
}

/* ---- several meshers, one job: the device sink's side of mlsgpu_amd/dist_sink.py (see include/mlsgpu_hip.h) ---- */
MLSGPU_API int mlsgpu_hip_mesher_boundary(mlsgpu_mesher *m, uint64_t *numKeys, uint64_t *numRoots)
{
    REQUIRE(m != nullptr && numKeys != nullptr && numRoots != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    m->bKeys.clear();
    m->bKeyRoot.clear();
    m->bRootVertices.clear();
    m->bRootTriangles.clear();
    m->analyzed = true;
    SinkSizes z;
    SinkScratch L;
    SinkCache had;
    PROPAGATE(m->begin(z, L, had));
    if (!z.empty())
    {
        /* behind an export or a plain finalize over the same arenas, the weld and the components are in the slab */
        uint32_t rootCount = 0;
        PROPAGATE(m->analyse(L, z, had.kind != SinkCache::None));
        PROPAGATE(m->numberRoots(L, z, &rootCount));
        PROPAGATE(m->checkUnion(L));
        PROPAGATE(m->exportBoundary(L, z, rootCount));
        m->cache = SinkCache{SinkCache::AfterExport, L.sortedInA, z.nv, z.nt, z.ne, rootCount};
    }
    *numKeys = m->bKeys.size();
    *numRoots = m->bRootVertices.size();
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesher_boundary_read(mlsgpu_mesher *m, uint64_t *keys, uint32_t *keyRoot, uint64_t *rootVertices,
                                               uint64_t *rootTriangles)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->analyzed, MLSGPU_ERR_INVALID);
    REQUIRE((m->bKeys.empty() || (keys != nullptr && keyRoot != nullptr))
            && (m->bRootVertices.empty() || (rootVertices != nullptr && rootTriangles != nullptr)), MLSGPU_ERR_INVALID);
    std::copy(m->bKeys.begin(), m->bKeys.end(), keys);
    std::copy(m->bKeyRoot.begin(), m->bKeyRoot.end(), keyRoot);
    std::copy(m->bRootVertices.begin(), m->bRootVertices.end(), rootVertices);
    std::copy(m->bRootTriangles.begin(), m->bRootTriangles.end(), rootTriangles);
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesher_finalize_with(mlsgpu_mesher *m, const uint8_t *keepRoot, uint64_t numRoots, uint32_t *numChunks)
{
    REQUIRE(m != nullptr && (numRoots == 0 || keepRoot != nullptr), MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->analyzed, MLSGPU_ERR_INVALID);
    SinkSizes z;
    SinkScratch L;
    SinkCache had;
    PROPAGATE(m->begin(z, L, had));
    if (z.empty())
        return m->finish(numChunks);
    /* right behind an export, weld, components and root numbering are still in the slab; this call leaves no record */
    const bool cached = had.kind == SinkCache::AfterExport;
    uint32_t rootCount = had.rootCount;
    PROPAGATE(m->analyse(L, z, cached));
    if (!cached)
        PROPAGATE(m->numberRoots(L, z, &rootCount));
    PROPAGATE(m->applyVerdict(L, rootCount, keepRoot, numRoots));
    PROPAGATE(m->writeOutput(L, z, 0.0, 1));        /* the "sizes" are all or nothing now */
    /* this mesher's own part of the job: kept components and their welded vertices from the export */
    m->stats[4] = 0;
    for (uint64_t r = 0; r < numRoots; r++)
        if (keepRoot[r])
            m->stats[4] += m->bRootVertices[r];
    return m->finish(numChunks);
}

namespace
{
std::string plyHeader(uint64_t numVertices, uint64_t numTriangles, const char *const *comments, uint32_t numComments,
                      bool normals = false)
{
    std::string head = "ply\nformat binary_little_endian 1.0\n";
    for (uint32_t i = 0; i < numComments; i++)
        head += std::string("comment ") + comments[i] + "\n";
    head += "element vertex " + std::to_string(numVertices) + "\nproperty float32 x\nproperty float32 y\nproperty float32 z\n";
    if (normals)
        head += "property float32 nx\nproperty float32 ny\nproperty float32 nz\n";
    head += "element face " + std::to_string(numTriangles) + "\nproperty list uint8 uint32 vertex_indices\ncomment padding:";
    size_t size = head.size() + 12;
    while (size % 4 != 0)
    {
        head += 'X';
        size++;
    }
    head += "\nend_header\n";
    return head;
}

/* a face of the file: the count byte and three indices, 13 bytes, packed on the device */
__global__ __launch_bounds__(256) void packFacesKernel(const uint32_t *triangles, uint64_t n, uint8_t *out)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    uint8_t *o = out + 13 * i;
    o[0] = 3;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const uint32_t v = triangles[3 * i + k];
        o[1 + 4 * k] = (uint8_t) v;
        o[2 + 4 * k] = (uint8_t) (v >> 8);
        o[3 + 4 * k] = (uint8_t) (v >> 16);
        o[4 + 4 * k] = (uint8_t) (v >> 24);
    }
}

/* a vertex of the file with normals: x y z nx ny nz, 24 bytes, interleaved on the device */
__global__ __launch_bounds__(256) void packVerticesKernel(const float *vertices, const float *normals, uint64_t n, float *out)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        out[6 * i + k] = vertices[3 * i + k];
        out[6 * i + 3 + k] = normals[3 * i + k];
    }
}
} // namespace

/*
 * One output chunk of a finalized mesher straight from HBM into FastPly::Writer's file, through two pinned buffers of
 * bufferBytes / 2: while one piece is written, the next travels (the role of src/async_io.h:95-140 behind the reference's
 * writer: the host never holds more of the mesh than the buffer).  Faces are packed into the file's 13-byte records on the
 * device.  The file is byte for byte what mlsgpu_hip_write_ply makes of the downloaded arrays.
 * withNormals: the chunk's normals (computed now if nobody asked for them yet) interleaved with its vertices into 24-byte
 * rows on the device, as the faces are packed; the file is mlsgpu_hip_write_ply_normals'.
 */
namespace
{
int writeChunkPly(mlsgpu_mesher *m, uint32_t i, const char *path, const char *const *comments, uint32_t numComments,
                  uint64_t bufferBytes, bool withNormals)
{
    REQUIRE(m != nullptr && path != nullptr, MLSGPU_ERR_INVALID);
    std::lock_guard<std::mutex> lock(m->mutex);
    REQUIRE(m->finalized && i < m->outChunks.size(), MLSGPU_ERR_INVALID);
    mlsgpu_ctx *ctx = m->ctx;
    HIP_CHECK(hipSetDevice(ctx->device));
    const uint32_t c = m->outChunks[i];
    const float *dN = nullptr;
    if (withNormals)
        PROPAGATE(m->chunkNormals(c, &dN, nullptr));
    const uint64_t rowBytes = withNormals ? 24 : 12;
    const uint64_t nv = m->span(c).nv, nt = m->span(c).nt;
    const uint8_t *dV = reinterpret_cast<const uint8_t *>(m->outVertices + 3 * m->span(c).v0);
    const uint32_t *dT = m->outTriangles + 3 * m->span(c).t0;
    if (bufferBytes == 0)
        bufferBytes = uint64_t(64) << 20;
    /* a piece holds whole 12-byte (with normals 24-byte) vertices and whole 13-byte faces */
    const uint64_t unit = 13 * rowBytes;
    const uint64_t piece = std::max<uint64_t>(bufferBytes / 2 / unit, 1) * unit;
    PinnedArray<uint8_t> pinned[2];
    DeviceArray<uint8_t> dPack;
    hipEvent_t done[2] = {nullptr, nullptr};
    FILE *f = nullptr;
    int rc = MLSGPU_OK;
    auto cleanup = [&]()
    {
        for (int k = 0; k < 2; k++)
            if (done[k]) hipEventDestroy(done[k]);
        if (f != nullptr)
            std::fclose(f);
    };
    for (int k = 0; k < 2 && rc == MLSGPU_OK; k++)
        if ((rc = pinned[k].alloc(piece)) == MLSGPU_OK && hipEventCreateWithFlags(&done[k], hipEventDisableTiming) != hipSuccess)
            rc = setError(MLSGPU_ERR_HIP, "mesher: cannot create an event");
    if (rc == MLSGPU_OK)
        rc = dPack.alloc(2 * piece);
    if (rc == MLSGPU_OK && (f = std::fopen(path, "wb")) == nullptr)
        rc = setError(MLSGPU_ERR_INVALID, "cannot open %s for writing", path);
    if (rc != MLSGPU_OK)
    {
        cleanup();
        return rc;
    }
    const std::string head = plyHeader(nv, nt, comments, numComments, withNormals);
    bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
    /* the pieces of the file body in order: vertex bytes, then face records; piece k + 1 is on its way while k is written */
    const uint64_t vBytes = rowBytes * nv, fBytes = 13 * nt, total = vBytes + fBytes;
    const uint64_t vPieces = (vBytes + piece - 1) / piece, fPieces = (fBytes + piece - 1) / piece, pieces = vPieces + fPieces;
    auto issue = [&](uint64_t k) -> hipError_t
    {
        const int slot = (int) (k & 1);
        if (k < vPieces)
        {
            const uint64_t off = k * piece, n = std::min(piece, vBytes - off);
            const uint8_t *from = dV + off;
            hipError_t e = hipSuccess;
            if (withNormals)
            {
                const uint64_t firstRow = off / 24, rows = n / 24;
                uint8_t *pack = dPack + (uint64_t) slot * piece;
                hipLaunchKernelGGL(packVerticesKernel, dim3(divUp(rows, 256)), dim3(256), 0, ctx->stream,
                                   reinterpret_cast<const float *>(dV) + 3 * firstRow, dN + 3 * firstRow, rows,
                                   reinterpret_cast<float *>(pack));
                e = hipGetLastError();
                from = pack;
            }
            if (e == hipSuccess)
                e = hipMemcpyAsync(pinned[slot], from, n, hipMemcpyDeviceToHost, ctx->stream);
            return e != hipSuccess ? e : hipEventRecord(done[slot], ctx->stream);
        }
        const uint64_t off = (k - vPieces) * piece, n = std::min(piece, fBytes - off);
        const uint64_t firstFace = off / 13, faces = n / 13;
        uint8_t *pack = dPack + (uint64_t) slot * piece;
        hipLaunchKernelGGL(packFacesKernel, dim3(divUp(faces, 256)), dim3(256), 0, ctx->stream, dT + 3 * firstFace, faces, pack);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(pinned[slot], pack, n, hipMemcpyDeviceToHost, ctx->stream);
        return e != hipSuccess ? e : hipEventRecord(done[slot], ctx->stream);
    };
    hipError_t e = pieces > 0 ? issue(0) : hipSuccess;
    uint64_t written = 0;
    for (uint64_t k = 0; k < pieces && ok && e == hipSuccess; k++)
    {
        if (k + 1 < pieces)
            e = issue(k + 1);
        if (e == hipSuccess)
            e = hipEventSynchronize(done[k & 1]);
        if (e != hipSuccess)
            break;
        const uint64_t n = k < vPieces ? std::min(piece, vBytes - k * piece) : std::min(piece, fBytes - (k - vPieces) * piece);
        ok = std::fwrite(pinned[k & 1], 1, n, f) == n;
        written += n;
    }
    hipStreamSynchronize(ctx->stream);
    ok = (std::fclose(f) == 0) && ok && written == total;
    f = nullptr;
    cleanup();
    if (e != hipSuccess)
        return setError(MLSGPU_ERR_HIP, "mesher: reading the mesh back failed: %s", hipGetErrorString(e));
    if (!ok)
        return setError(MLSGPU_ERR_INVALID, "writing %s failed", path);
    return MLSGPU_OK;
}
} // namespace

MLSGPU_API int mlsgpu_hip_mesher_write_ply(mlsgpu_mesher *m, uint32_t i, const char *path, const char *const *comments,
                                           uint32_t numComments, uint64_t bufferBytes)
{
    return writeChunkPly(m, i, path, comments, numComments, bufferBytes, false);
}

MLSGPU_API int mlsgpu_hip_mesher_write_ply_normals(mlsgpu_mesher *m, uint32_t i, const char *path, const char *const *comments,
                                                   uint32_t numComments, uint64_t bufferBytes)
{
    return writeChunkPly(m, i, path, comments, numComments, bufferBytes, true);
}

namespace
{
/* the faces of the file from host memory: uint8 3 + 3 x uint32 each */
bool writeFaces(FILE *f, const uint32_t *triangles, uint64_t numTriangles)
{
    bool ok = true;
    std::vector<unsigned char> faces;
    const uint64_t batch = 1 << 20;
    for (uint64_t first = 0; ok && first < numTriangles; first += batch)
    {
        const uint64_t n = std::min(batch, numTriangles - first);
        faces.resize(13 * n);
        for (uint64_t i = 0; i < n; i++)
        {
            faces[13 * i] = 3;
            std::memcpy(&faces[13 * i + 1], triangles + 3 * (first + i), 12);
        }
        ok = std::fwrite(faces.data(), 13, n, f) == n;
    }
    return ok;
}
} // namespace

/* FastPly::Writer's file (src/fast_ply.cpp:443-521): header padded to a multiple of 4, float32 x y z per vertex,
 * uint8 3 + 3 x uint32 per face; host memory in, one file out */
MLSGPU_API int mlsgpu_hip_write_ply(const char *path, const float *vertices, uint64_t numVertices, const uint32_t *triangles,
                                    uint64_t numTriangles, const char *const *comments, uint32_t numComments)
{
    REQUIRE(path != nullptr && (numVertices == 0 || vertices != nullptr) && (numTriangles == 0 || triangles != nullptr),
            MLSGPU_ERR_INVALID);
    const std::string head = plyHeader(numVertices, numTriangles, comments, numComments);
    FILE *f = std::fopen(path, "wb");
    if (f == nullptr)
        return setError(MLSGPU_ERR_INVALID, "cannot open %s for writing", path);
    bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
    ok = ok && std::fwrite(vertices, 12, numVertices, f) == numVertices;
    ok = ok && writeFaces(f, triangles, numTriangles);
    ok = (std::fclose(f) == 0) && ok;
    if (!ok)
        return setError(MLSGPU_ERR_INVALID, "writing %s failed", path);
    return MLSGPU_OK;
}

/* The same file with property float32 nx / ny / nz after z: 24-byte vertex rows */
MLSGPU_API int mlsgpu_hip_write_ply_normals(const char *path, const float *vertices, const float *normals, uint64_t numVertices,
                                            const uint32_t *triangles, uint64_t numTriangles, const char *const *comments,
                                            uint32_t numComments)
{
    REQUIRE(path != nullptr && (numVertices == 0 || (vertices != nullptr && normals != nullptr))
            && (numTriangles == 0 || triangles != nullptr), MLSGPU_ERR_INVALID);
    const std::string head = plyHeader(numVertices, numTriangles, comments, numComments, true);
    FILE *f = std::fopen(path, "wb");
    if (f == nullptr)
        return setError(MLSGPU_ERR_INVALID, "cannot open %s for writing", path);
    bool ok = std::fwrite(head.data(), 1, head.size(), f) == head.size();
    const uint64_t batch = 1 << 20;
    std::vector<float> rows;
    for (uint64_t first = 0; ok && first < numVertices; first += batch)
    {
        const uint64_t n = std::min(batch, numVertices - first);
        rows.resize(6 * n);
        for (uint64_t i = 0; i < n; i++)
        {
            std::memcpy(&rows[6 * i], vertices + 3 * (first + i), 12);
            std::memcpy(&rows[6 * i + 3], normals + 3 * (first + i), 12);
        }
        ok = std::fwrite(rows.data(), 24, n, f) == n;
    }
    ok = ok && writeFaces(f, triangles, numTriangles);
    ok = (std::fclose(f) == 0) && ok;
    if (!ok)
        return setError(MLSGPU_ERR_INVALID, "writing %s failed", path);
    return MLSGPU_OK;
}
