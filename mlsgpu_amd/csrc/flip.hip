/*
 * Delaunay edge flips of an indexed triangle mesh that is resident in HBM, with a triangle quality report.  The reference has
 * no counterpart: its meshes leave the device as marching made them, needles and caps included.  The contract
 * (include/mlsgpu_hip.h, DESIGN.md "Mesh edge flips") is written so that every output is a count, a minimum, a maximum or a
 * row that one deterministic winner writes: the result depends neither on the schedule nor on how the triangles are ordered.
 *
 *   check      a thread per vertex: the coordinates that are not finite
 *   quality    over the triangles, before the first round and after the last: classes, histogram, the smallest q
 *   per classification:
 *     records  a thread per triangle: its three directed sides as keys from << b | to (dead ones for a triangle that takes
 *              no part); the sort numbers them, so a record's value is 3 * triangle + corner
 *     sort     the keys: equal sides become one run, the sides that leave a vertex one segment
 *     segments a thread per record: where each vertex's segment starts and ends, so that a side's reverse and the sides of
 *              guard (i) are searched among the few sides that leave one vertex, not among all records
 *     classify over the records, at the head of a run a -> b, a < b, that is alone and whose reverse is alone: the quad, P,
 *              the guards; a candidate's P, partner record and opposite vertices go to the record's slot, and P is raised
 *              into the best priority of its four vertices (lanes that share a vertex send once)
 *                                                                                     } one read-back: the counts
 *   per round:
 *     keys     a thread per record: a candidate that holds a vertex's best P lowers that vertex's best key to its own
 *     apply    over the records: a candidate that holds all four of its vertices rewrites its two rows
 *
 * check, quality, records, segments and the search for a side are in meshedges.hpp, which collapse.hip shares.
 *
 * classify reads the triangles and writes none; apply writes them and reads none (what it needs of the quad was stored), so
 * no kernel races with itself.  An index >= V is compared and counted, never used as an address; no address depends on a
 * coordinate.
 *
 * Scratch belongs to the call: 96 bytes per triangle (three records: the two sides of the sort's keys 48 and values 24 -- the
 * free side holds priority and partner --, the opposite vertices 24), 24 bytes per vertex (best priority, best key, segment),
 * and the sort's histogram (4 KB per 4096 records).
 */
#include "meshedges.hpp"

using namespace mlsgpu;

namespace
{

enum
{
    C_NON_FINITE = 0,           /* input coordinates */
    C_FLIPS = 1,                /* winners of all rounds */
    /* of one classification: cleared before each */
    C_EDGES = 2,
    C_INTERIOR = 3,
    C_NON_DELAUNAY = 4,
    C_BLOCKED = 5,
    C_CANDIDATES = 6,
    C_WORDS = 7,
    /* and a quality report's block (meshedges.hpp) before and after */
    ALL_WORDS = C_WORDS + 2 * Q_WORDS
};

/* step 4: the cotangent of the angle at p between q and r */
__device__ __forceinline__ double cotAt(const D3 &p, const D3 &q, const D3 &r)
{
    const D3 u = q - p, v = r - p, x = cross(u, v);
    return dot(u, v) / sqrt(dot(x, x));
}

/* what classify leaves per record for the round's kernels */
struct Slots
{
    uint64_t *priority;         /* the bits of a candidate's P (positive, so they order as P does); 0 for every other record */
    uint32_t *partner;          /* a candidate's reverse record b -> a */
    uint2 *opposite;            /* a candidate's c and d */
};

/* The lanes that are `on` raise best[vertex] to their bits; lanes that share the vertex send once (a hub of valence 10^4 has
 * all its spokes on one address).  Needs the full wave. */
__device__ __forceinline__ void raiseBest(bool on, uint32_t vertex, uint64_t bits, Counter *best)
{
    forEachRoot(on, vertex, [&](uint32_t root, bool same, uint64_t sharers, bool leads) {
        const uint64_t most = (sharers & (sharers - 1)) == 0 ? bits : waveMax64(same ? bits : 0);
        if (leads)
            atomicMax(&best[root], (Counter) most);
    });
}

/* Steps 2 to 5.  The record at the head of a run speaks for its side.  An edge is counted by its falling side, or by its
 * rising one where that finds no falling side: only the rising sides search.  A workgroup loops over the records in whole
 * blocks -- every lane stays to the end, raiseBest needs the full wave -- and sends its five counts once (fewer than 2^32
 * records: they fit 32 bits). */
__global__ __launch_bounds__(256) void classifyKernel(Records R, const uint2 *run, const float *vertices, const uint32_t *tri,
                                                      double minGain, double minCos, Slots S, Counter *bestPriority, Counter *counters)
{
    __shared__ GroupCounts<5> sums;
    sums.clear();
    const int at[5] = {C_EDGES, C_INTERIOR, C_NON_DELAUNAY, C_BLOCKED, C_CANDIDATES};
    uint32_t count[5] = {0, 0, 0, 0, 0};
    const uint32_t n = (uint32_t) R.n;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < R.n; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        uint64_t bits = 0;
        uint32_t a = 0, b = 0, c = 0, d = 0, reverse = 0;
        const uint64_t key = i < R.n ? R.keys[i] : R.dead();
        if (R.fromOf(key) < R.numVertices && R.head(i, key))
        {
            a = (uint32_t) R.fromOf(key);
            b = R.toOf(key);
            reverse = a < b ? sideOf(R, run, b, a) : n;
            count[0] += reverse == n ? 1u : 0u;
            if (reverse != n && R.single(i, key) && R.single(reverse, R.keyOf(b, a)))
            {
                const uint32_t s1 = R.vals[i], s2 = R.vals[reverse];            /* 3 * triangle + the corner the side leaves */
                c = tri[s1 - s1 % 3 + (s1 + 2) % 3];
                d = tri[s2 - s2 % 3 + (s2 + 2) % 3];
                if (c != d)
                {
                    count[1]++;
                    const D3 pa = vertexAt(vertices, a), pb = vertexAt(vertices, b);
                    const D3 pc = vertexAt(vertices, c), pd = vertexAt(vertices, d);
                    const double P = -(cotAt(pc, pa, pb) + cotAt(pd, pb, pa));
                    if (P > minGain)
                    {
                        count[2]++;
                        const D3 n1 = face(pa, pb, pc), n2 = face(pb, pa, pd), N = n1 + n2;
                        const D3 m1 = face(pa, pd, pc), m2 = face(pb, pc, pd);
                        const bool flat = dot(n1, n2) >= (minCos * sqrt(dot(n1, n1))) * sqrt(dot(n2, n2));
                        const bool convex = dot(m1, N) > 0.0 && dot(m2, N) > 0.0;
                        if (flat && convex && sideOf(R, run, c, d) == n && sideOf(R, run, d, c) == n)
                        {
                            count[4]++;
                            bits = (uint64_t) __double_as_longlong(P);
                        }
                        else
                            count[3]++;
                    }
                }
            }
        }
        if (i < R.n)
        {
            S.priority[i] = bits;
            S.partner[i] = reverse;
            S.opposite[i] = make_uint2(c, d);
        }
        const uint32_t corner[4] = {a, b, c, d};
#pragma unroll
        for (int k = 0; k < 4; k++)     /* the word is read first: most lanes of a hub find a larger P there already */
            raiseBest(bits != 0 && bits > loadWord(&bestPriority[corner[k]]), corner[k], bits, bestPriority);
    }
#pragma unroll
    for (int k = 0; k < 5; k++)
        sums.add(k, count[k]);
    sums.flush(counters, at);
}

/* step 6, the tie: among the candidates that hold a vertex's best P the smallest key.  Few lanes get this far -- one per vertex
 * and tie -- and the word is read first. */
__global__ __launch_bounds__(256) void keysKernel(Records R, Slots S, const Counter *bestPriority, Counter *bestKey)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n)
        return;
    const uint64_t bits = S.priority[i];
    if (bits == 0)
        return;
    const uint64_t key = R.keys[i];
    const uint2 cd = S.opposite[i];
    const uint32_t corner[4] = {(uint32_t) R.fromOf(key), R.toOf(key), cd.x, cd.y};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (bestPriority[corner[k]] == bits && key < loadWord(&bestKey[corner[k]]))
            atomicMin(&bestKey[corner[k]], (Counter) key);
}

/* Steps 6 and 7.  A winner holds all four of its vertices, so no other winner names its triangles.  A workgroup loops over the
 * records and sends its count once. */
__global__ __launch_bounds__(256) void applyKernel(Records R, Slots S, const Counter *bestPriority, const Counter *bestKey,
                                                   uint32_t *tri, Counter *counters)
{
    __shared__ GroupCounts<1> sums;
    sums.clear();
    const int at[1] = {C_FLIPS};
    uint32_t winners = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < R.n; i += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t bits = S.priority[i];
        if (bits == 0)
            continue;
        const uint64_t key = R.keys[i];
        const uint2 cd = S.opposite[i];
        const uint32_t a = (uint32_t) R.fromOf(key), b = R.toOf(key), c = cd.x, d = cd.y;
        const uint32_t corner[4] = {a, b, c, d};
        bool wins = true;
#pragma unroll
        for (int k = 0; k < 4; k++)
            wins = wins && bestPriority[corner[k]] == bits && bestKey[corner[k]] == key;
        if (!wins)
            continue;
        const uint64_t t1 = R.vals[i] / 3, t2 = R.vals[S.partner[i]] / 3;
        tri[3 * t1] = a;
        tri[3 * t1 + 1] = d;
        tri[3 * t1 + 2] = c;
        tri[3 * t2] = b;
        tri[3 * t2 + 1] = c;
        tri[3 * t2 + 2] = d;
        winners++;
    }
    sums.add(0, winners);
    sums.flush(counters, at);
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_flip_edges(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices,
                                          const uint32_t *dTriangles, uint64_t numTriangles, uint32_t maxRounds, double minGain,
                                          double minCos, uint32_t *dOutTriangles, mlsgpu_flip_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(minGain) && minGain >= 0.0 && minCos >= -1.0 && minCos <= 1.0, MLSGPU_ERR_INVALID);
    /* the sort's values and tile counts are 32-bit, and so are the indices of a triangle: 3 T < 2^32 */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || dVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || (dTriangles != nullptr && dOutTriangles != nullptr), MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->numVertices = numVertices;
    stats->numTriangles = numTriangles;
    if ((numVertices == 0 || numTriangles == 0) && maxRounds > 0)
        stats->rounds = stats->converged = 1;   /* no triangle takes part: the first round finds no winner */
    if (numVertices == 0 && numTriangles == 0)
        return MLSGPU_OK;

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t nv = numVertices, nt = numTriangles, n = 3 * nt;
    const dim3 B(256);
    if (nt > 0 && dOutTriangles != dTriangles)
        HIP_CHECK(hipMemcpyAsync(dOutTriangles, dTriangles, nt * 12, hipMemcpyDeviceToDevice, ctx->stream));
    if (nv == 0)
    {
        stats->outOfRangeTriangles = nt;        /* every index is >= 0 vertices: the rows keep their bits */
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MLSGPU_OK;
    }

    const SideKeys K = SideKeys::of(nv);
    DeviceArray<Counter> counters, best;
    DeviceArray<uint2> opposite, run;
    SortScratch sides;
    PROPAGATE(counters.alloc(ALL_WORDS));
    double scratch = (double) counters.bytes(ALL_WORDS);
    if (nt > 0)
    {
        PROPAGATE(best.alloc(2 * nv));
        PROPAGATE(opposite.alloc(n));
        PROPAGATE(run.alloc(nv));
        PROPAGATE(sides.alloc(n));
        scratch += (double) (best.bytes(2 * nv) + run.bytes(nv) + opposite.bytes(n) + sides.bytes());
    }
    if (ctx->timing)
        ctx->addValue("flip.scratch.bytes", scratch);
    Counter *const bestPriority = best.get(), *const bestKey = best.get() + nv;
    Counter *const before = counters.get() + C_WORDS, *const after = before + Q_WORDS;

    Counter h[ALL_WORDS];
    HIP_CHECK(hipMemsetAsync(counters.get(), 0, sizeof(h), ctx->stream));
    LAUNCH(ctx, "kernel.flip.check", checkKernel, dim3(divUp(nv, 256)), B, dVertices, nv, counters.get() + C_NON_FINITE);
    if (nt > 0)
        LAUNCH(ctx, "kernel.flip.quality", qualityKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, dVertices, nv,
               (const uint32_t *) dOutTriangles, nt, before);
    /* step 8 */
    for (bool first = true; nt > 0; first = false)
    {
        HIP_CHECK(hipMemsetAsync(counters.get() + C_EDGES, 0, (C_WORDS - C_EDGES) * sizeof(Counter), ctx->stream));
        HIP_CHECK(hipMemsetAsync(bestPriority, 0, nv * sizeof(Counter), ctx->stream));
        HIP_CHECK(hipMemsetAsync(bestKey, 0xFF, nv * sizeof(Counter), ctx->stream));
        LAUNCH(ctx, "kernel.flip.records", recordsKernel, dim3(divUp(nt, 256)), B, (const uint32_t *) dOutTriangles, nt, K, sides.keys());
        Records R;
        PROPAGATE(sides.sort(ctx, "kernel.flip.sort", K, true, &R));
        /* the side of the sort that is free again: a 64-bit and a 32-bit word per record */
        const Slots S{sides.freeKeys(), sides.freeVals(), opposite.get()};
        LAUNCH(ctx, "kernel.flip.segments", segmentsKernel, dim3(divUp(n, 256)), B, R, run.get());
        LAUNCH(ctx, "kernel.flip.classify", classifyKernel, dim3(std::min(divUp(n, 256), LOOP_BLOCKS)), B, R, (const uint2 *) run.get(),
               dVertices, (const uint32_t *) dOutTriangles, minGain, minCos, S, bestPriority, counters.get());
        HIP_CHECK(hipMemcpyAsync(h, counters.get(), C_WORDS * sizeof(Counter), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (h[C_NON_FINITE] != 0)
            break;
        if (first)
        {
            stats->numEdges = h[C_EDGES];
            stats->interiorEdges = h[C_INTERIOR];
            stats->nonDelaunayBefore = h[C_NON_DELAUNAY];
        }
        stats->nonDelaunayAfter = h[C_NON_DELAUNAY];
        stats->blockedAfter = h[C_BLOCKED];
        if (stats->rounds == maxRounds)
            break;
        stats->rounds++;
        if (h[C_CANDIDATES] == 0)       /* the best candidate of the mesh always wins: no candidate, no winner */
        {
            stats->converged = 1;
            break;
        }
        LAUNCH(ctx, "kernel.flip.keys", keysKernel, dim3(divUp(n, 256)), B, R, S, (const Counter *) bestPriority, bestKey);
        LAUNCH(ctx, "kernel.flip.apply", applyKernel, dim3(std::min(divUp(n, 256), LOOP_BLOCKS)), B, R, S,
               (const Counter *) bestPriority, (const Counter *) bestKey, dOutTriangles, counters.get());
    }
    if (nt > 0)
        LAUNCH(ctx, "kernel.flip.quality", qualityKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, dVertices, nv,
               (const uint32_t *) dOutTriangles, nt, after);
    HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h[C_NON_FINITE] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh flip edges: %llu vertices have a coordinate that is not finite", h[C_NON_FINITE]);

    stats->flips = h[C_FLIPS];
    stats->outOfRangeTriangles = h[C_WORDS + Q_OUT_OF_RANGE];
    stats->degenerateTriangles = h[C_WORDS + Q_DEGENERATE];
    qualityOut(h + C_WORDS, &stats->minQualityBefore, stats->qualityBefore);
    qualityOut(h + C_WORDS + Q_WORDS, &stats->minQualityAfter, stats->qualityAfter);
    return MLSGPU_OK;
}
