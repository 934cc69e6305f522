/*
 * Repair of an indexed triangle mesh that is resident in HBM: triangles with a repeated directed side are dropped and
 * pinched vertices are split, so that what mlsgpu_hip_mesh_topology calls non-manifold -- after a simplify, say -- becomes an
 * oriented manifold with boundary again, as the reference guarantees for everything it writes.  The contract
 * (include/mlsgpu_hip.h, DESIGN.md "Repair") is written so that every result is a count, a minimum or a scan: the output
 * depends neither on the schedule nor on how the triangles are ordered.
 *
 *   sides      a thread per triangle: its state (kept so far, or bad), and its three directed sides as keys from << b | to;
 *              the sort numbers the records, so record 3 t + j is corner j of triangle t
 *   sort       the keys: the sides that leave a vertex become one segment, equal sides one run
 *   runs       over the records: the triangles of a run longer than one are dropped (a store of 1); every vertex's segment
 *   twins      over the records of kept triangles: a binary search for to -> from in to's segment.  If a kept triangle has
 *              it, the two corners at `from` are united in a forest over the 3 T corners (unionfind.hpp); if not, the side is
 *              open
 *   marks      over the same records: the corner's root -- the smallest corner of its umbrella, whatever the schedule --
 *              gets the smallest `to` of the umbrella and, from an open side, the chain flag
 *   umbrellas  an umbrella's leader is the record whose `to` is the root's minimum: it counts the umbrella at its vertex as a
 *              ring or a chain, and lowers the vertex's smallest chain key and smallest key
 *   heads      over the records: a group's head is the record whose `to` is the group's key; the counts of the statistics
 *                                                                                                        -- one read-back --
 *   vertices   a scan over the records with the flag at the heads: they lie in (from, to) order, which is the (v, key) order
 *              of the contract, so the scan numbers the output vertices; a head copies its vertex's 12 bytes
 *   triangles  a scan over the triangles with the flag at the kept ones; a corner finds its group's head in its vertex's
 *              segment and takes its number
 *
 * No kernel walks an umbrella or a vertex's segment: a hub of degree 10^5 costs what 10^5 other corners cost (meshpost.hpp's
 * forEachRoot combines the lanes of a wave that share a root or a vertex).  An index >= V is compared and counted, never
 * used as an address; positions are copied as bits, never computed with.
 *
 * Scratch belongs to the call: 97 bytes per triangle (three records: the two sides of the sort's 64-bit keys and 32-bit
 * values -- the side the sort leaves free holds the umbrellas' minima, the heads' numbers and the records' flags --, the
 * corner forest's parent 12, the chain flags 12, the triangle's state 1), 24 bytes per vertex (segment start and end, ring
 * and chain count, smallest chain key, smallest key), the sort's histogram and the scan's tile sums.
 */
#include "meshpost.hpp"
#include "unionfind.hpp"

using namespace mlsgpu;

namespace
{

enum
{
    C_OUT_OF_RANGE = 0,
    C_DEGENERATE = 1,
    C_REPEATED = 2,             /* records in runs longer than one */
    C_DROPPED = 3,              /* triangles with such a record */
    C_USED = 4,                 /* vertices a kept triangle uses */
    C_SPLIT = 5,                /* ... with more than one group */
    C_HEADS = 6,                /* groups = output vertices */
    C_FAILED = 7,               /* the union-find's retry bound was reached (its low 32 bits are the flag) */
    C_WORDS = 8
};

/* a triangle's state: sides writes KEPT or BAD, runs overwrites KEPT with DROPPED */
enum : uint8_t
{
    T_KEPT = 0,
    T_DROPPED = 1,
    T_BAD = 2
};

/* a record's flags */
enum
{
    R_OPEN = 1,                 /* the side of a kept triangle without a kept twin */
    R_HEAD = 2                  /* the head of its group */
};

const uint32_t NONE = 0xFFFFFFFFu;      /* above every vertex: what a minimum starts from */

/* LOOP_BLOCKS for the twins kernel, which waits for its binary searches: more waves in flight */
const uint32_t TWINS_BLOCKS = 4096;

/* the smallest value of the wave, in every lane (a FULL wave, as for waveMax) */
__device__ __forceinline__ uint32_t waveMin(uint32_t v) { return ~waveMax(~v); }

/* What the umbrellas kernel leaves, and step 4 of the contract on it: the key of the group that a corner with root `root`
 * at vertex v belongs to. */
struct Groups
{
    const uint32_t *parent;     /* corner -> its root, once the marks kernel has run */
    const uint32_t *minTo;      /* at a root: the smallest `to` of the umbrella */
    const uint32_t *chain;      /* at a root: non-zero for a chain */
    const uint32_t *ringCount, *chainCount, *chainMin, *allMin;         /* per vertex */
    uint32_t pinches;           /* MLSGPU_REPAIR_SPLIT_PINCHES */

    /* the reference's check fails at v: a ring, and another umbrella */
    __device__ __forceinline__ bool mixed(uint64_t v) const
    {
        const uint32_t rings = ringCount[v];
        return rings >= 1 && rings + chainCount[v] > 1;
    }
    __device__ __forceinline__ bool split(uint64_t v) const { return pinches ? ringCount[v] + chainCount[v] > 1 : mixed(v); }
    __device__ __forceinline__ uint32_t keyOf(uint64_t v, uint32_t root) const
    {
        if (pinches)
            return minTo[root];
        if (mixed(v))
            return chain[root] != 0 ? chainMin[v] : minTo[root];
        return allMin[v];
    }
};

__global__ __launch_bounds__(256) void identityKernel(uint32_t *parent, uint64_t n)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        parent[i] = (uint32_t) i;
}

/* Step 1: the three directed sides of a triangle; three dead records for a bad one */
__global__ __launch_bounds__(256) void sidesKernel(const uint32_t *tri, uint64_t numTriangles, SideKeys K, uint64_t *keys, uint8_t *state,
                                                   Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    const TriangleDefect d = defectOf(i, K.numVertices);
    tally(d.outOfRange, &counters[C_OUT_OF_RANGE]);
    tally(d.degenerate, &counters[C_DEGENERATE]);
    state[t] = d.none() ? T_KEPT : T_BAD;
#pragma unroll
    for (int k = 0; k < 3; k++)
        keys[3 * t + k] = d.none() ? K.keyOf(i[k], i[k == 2 ? 0 : k + 1]) : K.dead();
}

/* Step 2.  Every record of a run longer than one stores the same 1 into its triangle's state, whichever comes first.  The
 * first and the last record of a vertex's segment write its bounds: every vertex of a live triangle has a side out, so every
 * vertex that is looked up later has them.  A workgroup loops over the records and sends its count once: after a fine
 * simplify most waves hold a repeated side, and one atomic per such wave made this kernel 0.095 ms on a 695 480-triangle chunk
 * (profiles/NOTES_repair.md). */
__global__ __launch_bounds__(256) void runsKernel(Records R, uint8_t *state, uint32_t *segStart, uint32_t *segEnd, Counter *counters)
{
    __shared__ GroupCounts<1> repeats;
    repeats.clear();
    const int at[1] = {C_REPEATED};
    uint32_t count = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < R.n; i += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t key = R.keys[i], from = R.fromOf(key);
        if (from >= R.numVertices)
            continue;           /* the record of a bad triangle */
        if (!R.single(i, key))
        {
            count++;
            state[R.vals[i] / 3] = T_DROPPED;
        }
        if (R.segmentStart(i, from))
            segStart[from] = (uint32_t) i;
        if (R.segmentEnd(i, from))
            segEnd[from] = (uint32_t) i + 1;
    }
    repeats.add(0, count);
    repeats.flush(counters, at);
}

/* Step 3.  The states are final (a launch lies between).  The side from -> to of corner c of a kept triangle: if a kept
 * triangle has to -> from at its corner c2 -- at `to` --, its next corner lies at `from` and belongs with c.  A kept
 * triangle's records are alone in their runs, so the first record with the key is the only candidate. */
__global__ __launch_bounds__(256) void twinsKernel(Records R, const uint8_t *state, const uint32_t *segStart, const uint32_t *segEnd,
                                                   uint32_t *parent, uint32_t *info, Counter *counters)
{
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < R.n; i += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t key = R.keys[i], from = R.fromOf(key);
        if (from >= R.numVertices)
            continue;
        const uint32_t c = R.vals[i];
        if (state[c / 3] != T_KEPT)
            continue;
        const uint32_t to = R.toOf(key);
        const uint32_t end = segEnd[to], p = R.find(segStart[to], end, R.keyOf(to, from));
        bool twin = false;
        if (p != end)
        {
            const uint32_t c2 = R.vals[p], t2 = c2 / 3;
            if (state[t2] == T_KEPT)
            {
                twin = true;
                const uint32_t j2 = c2 - 3 * t2;
                unite(parent, c, 3 * t2 + (j2 == 2 ? 0 : j2 + 1), reinterpret_cast<uint32_t *>(&counters[C_FAILED]), UNION_SHORTCUT);
            }
        }
        if (!twin)
            info[i] = R_OPEN;
    }
}

/* the record i of a kept triangle, for the kernels behind the unions: every lane of a workgroup loops as often, so that the
 * wave is whole where its lanes talk */
struct KeptRecord
{
    bool on;
    uint32_t corner, to;
    uint64_t from;
    __device__ __forceinline__ KeptRecord(const Records &R, const uint8_t *state, uint64_t i) : on(false), corner(0), to(NONE), from(0)
    {
        if (i >= R.n)
            return;
        const uint64_t key = R.keys[i];
        from = R.fromOf(key);
        if (from >= R.numVertices)
            return;
        corner = R.vals[i];
        to = R.toOf(key);
        on = state[corner / 3] == T_KEPT;
    }
};

/* The forest is finished: a root is its umbrella's smallest corner.  Every corner is re-parented to its root, for the kernels
 * behind this one; a walk of another thread that passes through it meanwhile meets the old parent or the root, both its
 * ancestors.  The lanes of the wave that share a root -- a vertex's records are neighbours -- send ONE minimum and at most one
 * flag. */
__global__ __launch_bounds__(256) void marksKernel(Records R, const uint8_t *state, const uint32_t *info, uint32_t *parent, uint32_t *minTo,
                                                   uint32_t *chain)
{
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < R.n; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        const KeptRecord k(R, state, i);
        uint32_t root = 0;
        bool open = false;
        if (k.on)
        {
            root = findRoot(parent, k.corner);
            __hip_atomic_store(&parent[k.corner], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            open = (info[i] & R_OPEN) != 0;
        }
        forEachRoot(k.on, root, [&](uint32_t r, bool same, uint64_t, bool leads) {
            const uint32_t least = waveMin(same ? k.to : NONE);
            const bool anyOpen = __ballot(same && open) != 0;
            if (leads)
            {
                atomicMin(&minTo[r], least);
                if (anyOpen)
                    chain[r] = 1;
            }
        });
    }
}

/* parent[] holds roots now, minTo[] and chain[] are complete.  An umbrella's leader -- directed sides are unique among the
 * kept triangles, so there is exactly one -- counts it at its vertex; the leaders of a vertex in one wave send together. */
__global__ __launch_bounds__(256) void umbrellasKernel(Records R, const uint8_t *state, const uint32_t *parent, const uint32_t *minTo,
                                                       const uint32_t *chain, uint32_t *ringCount, uint32_t *chainCount, uint32_t *chainMin,
                                                       uint32_t *allMin)
{
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < R.n; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const KeptRecord k(R, state, base + threadIdx.x);
        bool leader = false, isChain = false;
        if (k.on)
        {
            const uint32_t root = parent[k.corner];
            leader = k.to == minTo[root];
            isChain = leader && chain[root] != 0;
        }
        forEachRoot(leader, (uint32_t) k.from, [&](uint32_t v, bool same, uint64_t, bool leads) {
            const uint32_t chains = (uint32_t) __popcll(__ballot(same && isChain));
            const uint32_t rings = (uint32_t) __popcll(__ballot(same && !isChain));
            const uint32_t least = waveMin(same ? k.to : NONE), leastChain = waveMin(same && isChain ? k.to : NONE);
            if (leads)
            {
                if (rings != 0)
                    atomicAdd(&ringCount[v], rings);
                if (chains != 0)
                {
                    atomicAdd(&chainCount[v], chains);
                    atomicMin(&chainMin[v], leastChain);
                }
                atomicMin(&allMin[v], least);
            }
        });
    }
}

/* Steps 4 and 5, and the statistics.  The per-vertex words are complete.  A group's head is the record whose `to` is the
 * group's key; a vertex is counted at the record with its smallest `to`, a dropped triangle at its corner 0.  A workgroup
 * sends its four counts once (each is at most the records it looped over, fewer than 2^32 in the whole launch). */
__global__ __launch_bounds__(256) void headsKernel(Records R, const uint8_t *state, Groups G, uint32_t *info, Counter *counters)
{
    enum { DROPPED, USED, SPLIT, HEADS, COUNTS };
    const int at[COUNTS] = {C_DROPPED, C_USED, C_SPLIT, C_HEADS};
    __shared__ GroupCounts<COUNTS> totals;
    totals.clear();
    uint32_t count[COUNTS] = {0, 0, 0, 0};
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < R.n; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        const KeptRecord k(R, state, i);
        if (k.on)
        {
            if (k.to == G.keyOf(k.from, G.parent[k.corner]))
            {
                info[i] |= R_HEAD;
                count[HEADS]++;
            }
            if (k.to == G.allMin[k.from])
            {
                count[USED]++;
                count[SPLIT] += G.split(k.from) ? 1u : 0u;
            }
        }
        else if (k.to != NONE && k.corner % 3 == 0 && state[k.corner / 3] == T_DROPPED)
            count[DROPPED]++;
    }
#pragma unroll
    for (int j = 0; j < COUNTS; j++)
        totals.add(j, count[j]);
    totals.flush(counters, at);
}

/* Step 5: the flag stands at every head ... */
struct HeadIn
{
    const uint32_t *info;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return (info[i] & R_HEAD) != 0 ? 1u : 0u; }
};
/* ... and the head writes its number, its vertex's position bits and the vertex itself */
struct HeadOut
{
    Records R;
    const uint32_t *vertices;   /* the positions as bits */
    uint32_t *rank, *outVertices, *outSource;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t before, uint32_t flag) const
    {
        if (!flag)
            return;
        rank[i] = before;
        const uint64_t v = R.fromOf(R.keys[i]);
#pragma unroll
        for (int k = 0; k < 3; k++)
            outVertices[3 * (uint64_t) before + k] = vertices[3 * v + k];
        if (outSource != nullptr)
            outSource[before] = (uint32_t) v;
    }
};

/* Step 6: the flag stands at every kept triangle; a corner at v finds the record v -> key of its group */
struct KeptIn
{
    const uint8_t *state;
    __device__ __forceinline__ uint32_t operator()(uint64_t t) const { return state[t] == T_KEPT ? 1u : 0u; }
};
struct TriangleOut
{
    Records R;
    Groups G;
    const uint32_t *tri, *segStart, *segEnd, *rank;
    uint32_t *outTriangles;
    __device__ __forceinline__ void operator()(uint64_t t, uint32_t before, uint32_t flag) const
    {
        if (!flag)
            return;
#pragma unroll
        for (int j = 0; j < 3; j++)
        {
            const uint64_t c = 3 * t + j, v = tri[c];
            const uint32_t key = G.keyOf(v, G.parent[c]), end = segEnd[v];
            const uint32_t head = R.find(segStart[v], end, R.keyOf(v, key));    /* there: the key is the `to` of a kept side of v */
            outTriangles[3 * (uint64_t) before + j] = head != end ? rank[head] : NONE;
        }
    }
};

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_repair(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                      uint64_t numTriangles, uint32_t flags, float *dOutVertices, uint64_t capVertices,
                                      uint32_t *dOutTriangles, uint64_t capTriangles, uint32_t *dOutSource, mlsgpu_repair_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE((flags & ~(uint32_t) MLSGPU_REPAIR_SPLIT_PINCHES) == 0, MLSGPU_ERR_INVALID);
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
    DeviceArray<Counter> counters;
    DeviceArray<uint32_t> parent, chain, perVertex, tileSums;
    DeviceArray<uint8_t> state;
    SortScratch records;
    Records R = Records{K, nullptr, 0, nullptr};
    Groups G = Groups();
    uint32_t *segStart = nullptr, *segEnd = nullptr, *info = nullptr, *rank = nullptr;
    Counter h[C_WORDS];
    std::memset(h, 0, sizeof(h));
    const bool sides = nv > 0 && nt > 0;        /* without vertices every triangle is out of range */
    if (sides)
    {
        const uint64_t tileElems = (uint64_t) scanTiles(n) + 1;
        PROPAGATE(counters.alloc(C_WORDS));
        PROPAGATE(parent.alloc(n));
        PROPAGATE(chain.alloc(n));
        PROPAGATE(state.alloc(nt));
        PROPAGATE(perVertex.alloc(6 * nv));
        PROPAGATE(tileSums.alloc(tileElems));
        PROPAGATE(records.alloc(n));
        if (ctx->timing)
            ctx->addValue("repair.scratch.bytes", (double) (counters.bytes(C_WORDS) + 2 * parent.bytes(n) + state.bytes(nt) + perVertex.bytes(6 * nv)
                                                            + tileSums.bytes(tileElems) + records.bytes()));
        segStart = perVertex.get();
        segEnd = segStart + nv;
        uint32_t *const ringCount = segEnd + nv, *const chainCount = ringCount + nv, *const chainMin = chainCount + nv, *const allMin = chainMin + nv;

        HIP_CHECK(hipMemsetAsync(counters.get(), 0, C_WORDS * sizeof(Counter), ctx->stream));
        HIP_CHECK(hipMemsetAsync(chain.get(), 0, n * sizeof(uint32_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(ringCount, 0, 2 * nv * sizeof(uint32_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(chainMin, 0xFF, 2 * nv * sizeof(uint32_t), ctx->stream));
        LAUNCH(ctx, "kernel.repair.init", identityKernel, dim3(divUp(n, 256)), B, parent.get(), n);
        LAUNCH(ctx, "kernel.repair.sides", sidesKernel, dim3(divUp(nt, 256)), B, dTriangles, nt, K, records.keys(), state.get(), counters.get());
        PROPAGATE(records.sort(ctx, "kernel.repair.sort", K, true, &R));
        /* the side the sort left free: per record the umbrella's minimum (at a root) and the head's number, and the flags */
        uint32_t *const minTo = reinterpret_cast<uint32_t *>(records.freeKeys());
        rank = minTo + n;
        info = records.freeVals();
        HIP_CHECK(hipMemsetAsync(minTo, 0xFF, n * sizeof(uint32_t), ctx->stream));
        HIP_CHECK(hipMemsetAsync(info, 0, n * sizeof(uint32_t), ctx->stream));
        G = Groups{parent.get(), minTo, chain.get(), ringCount, chainCount, chainMin, allMin, (flags & MLSGPU_REPAIR_SPLIT_PINCHES) != 0 ? 1u : 0u};

        const dim3 loop(std::min(divUp(n, 256), LOOP_BLOCKS));
        LAUNCH(ctx, "kernel.repair.runs", runsKernel, loop, B, R, state.get(), segStart, segEnd, counters.get());
        LAUNCH(ctx, "kernel.repair.twins", twinsKernel, dim3(std::min(divUp(n, 256), TWINS_BLOCKS)), B, R, (const uint8_t *) state.get(),
               (const uint32_t *) segStart, (const uint32_t *) segEnd, parent.get(), info, counters.get());
        LAUNCH(ctx, "kernel.repair.marks", marksKernel, loop, B, R, (const uint8_t *) state.get(), (const uint32_t *) info, parent.get(), minTo,
               chain.get());
        LAUNCH(ctx, "kernel.repair.umbrellas", umbrellasKernel, loop, B, R, (const uint8_t *) state.get(), (const uint32_t *) parent.get(),
               (const uint32_t *) minTo, (const uint32_t *) chain.get(), ringCount, chainCount, chainMin, allMin);
        LAUNCH(ctx, "kernel.repair.heads", headsKernel, loop, B, R, (const uint8_t *) state.get(), G, info, counters.get());
        HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    else if (nv == 0)
        h[C_OUT_OF_RANGE] = nt;         /* every index is >= 0 vertices */
    if ((uint32_t) h[C_FAILED] != 0)
        return setError(MLSGPU_ERR_HIP, "mesh repair: the union-find did not settle within its retry bound");

    stats->outOfRangeTriangles = h[C_OUT_OF_RANGE];
    stats->degenerateTriangles = h[C_DEGENERATE];
    stats->repeatedSides = h[C_REPEATED];
    stats->droppedTriangles = h[C_DROPPED];
    stats->unusedVertices = nv - h[C_USED];
    stats->splitVertices = h[C_SPLIT];
    stats->addedVertices = h[C_HEADS] - h[C_USED];
    stats->outVertices = h[C_HEADS];
    stats->outTriangles = nt - h[C_OUT_OF_RANGE] - h[C_DEGENERATE] - h[C_DROPPED];
    if (capVertices < stats->outVertices || capTriangles < stats->outTriangles)
        return setError(MLSGPU_ERR_LENGTH, "mesh repair: the outputs hold %llu vertices and %llu triangles, the repaired mesh has %llu and %llu",
                        (unsigned long long) capVertices, (unsigned long long) capTriangles, (unsigned long long) stats->outVertices,
                        (unsigned long long) stats->outTriangles);
    REQUIRE(stats->outVertices == 0 || dOutVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(stats->outTriangles == 0 || dOutTriangles != nullptr, MLSGPU_ERR_INVALID);

    if (stats->outTriangles > 0)        /* then there are heads too */
    {
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.repair.vertices", HeadIn{info},
                                           HeadOut{R, reinterpret_cast<const uint32_t *>(dVertices), rank,
                                                   reinterpret_cast<uint32_t *>(dOutVertices), dOutSource},
                                           n, 0u, tileSums.get(), (uint32_t *) nullptr)));
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.repair.triangles", KeptIn{state.get()},
                                           TriangleOut{R, G, dTriangles, segStart, segEnd, rank, dOutTriangles}, nt, 0u, tileSums.get(),
                                           (uint32_t *) nullptr)));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));   /* the scratch goes with the call */
    }
    return MLSGPU_OK;
}
