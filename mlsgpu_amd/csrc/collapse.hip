/*
 * Short-edge collapse of an indexed triangle mesh that is resident in HBM, with a triangle quality report.  Marching tetrahedra's
 * worst slivers have a short edge -- two vertices almost on top of each other where the surface passes close to a lattice
 * vertex --, which no flip takes out (profiles/NOTES_flip.md); a collapse does, where the needle is, and leaves everything else
 * bit for bit.  The reference has no counterpart.  The contract (include/mlsgpu_hip.h, DESIGN.md "Mesh edge collapse") is
 * written so that every output is a count, a minimum or something that one deterministic winner writes: the result depends
 * neither on the schedule nor on how the triangles are ordered.
 *
 *   check      a thread per vertex: the coordinates that are not finite                                  } meshedges.hpp
 *   quality    over the triangles, before the first round and after the last: classes, histogram, the smallest q
 *   per classification:
 *     records  a thread per triangle: its three directed sides as keys from << b | to (dead ones for a triangle that takes
 *              no part); the sort numbers them, so a record's value is 3 * triangle + corner          } meshedges.hpp
 *     sort     the keys: equal sides become one run, the sides that leave a vertex one segment
 *     segments a thread per record: where each vertex's segment starts and ends                        } meshedges.hpp
 *     fixed    over the records: the triangle's third vertex goes to the record's slot, so that the segment of x lists the
 *              triangles at x with both their other vertices and no kernel behind this one reads a row; the two ends of a
 *              side that is repeated or has no reverse are FIXED; the edges and the used vertices are counted
 *     classify over the records, at the head of a run a -> b, a < b, that is alone and whose reverse is alone: L2, and for a
 *              short edge the guards, by walking the segments of a and b (at most 64 records each: guard (ii)); a candidate's
 *              L2 goes to the record's slot and is lowered into the best L2 of every vertex of S
 *                                                                                     } one read-back: the counts
 *   per round:
 *     keys     a thread per record: a candidate that holds a vertex's best L2 lowers that vertex's best key to its own
 *     apply    over the records: a candidate that holds every vertex of its S writes the survivor into the rows of the
 *              removed vertex's triangles -- a record's value is the place of that corner -- and the survivor's position
 *   at the end:
 *     vertices a scan over the vertices with the flag at those that still have a segment: number, position bits, source
 *     triangles a scan over the triangles with the flag at those that still take part: the renumbered row
 *
 * classify and keys read the records, the slots and the positions and write none of them; apply writes rows and positions
 * only inside its winner's S, reads positions only of its own a and b, and winners have disjoint S: no kernel races with
 * itself.  The best words are lowered with the word read first (a stale read costs an atomic, never the result); guard (ii)
 * bounds how many candidates can name one vertex through its own triangles, and the ring around a larger hub, which all
 * name the hub, mostly finds a smaller L2 there already.  An index >= V is compared and counted, never used as an address.
 *
 * The inputs are left alone: rows and positions are copied into scratch first.  Scratch belongs to the call: 96 bytes per
 * triangle (three records: the two sides of the sort's 64-bit keys and 32-bit values 72 -- the free key side holds a
 * candidate's L2 --, the third vertices 12, and the copied row 12), 44 bytes per vertex (best L2 8, best key 8, segment 8,
 * fixed flag 4, copied position 12, output number 4), the sort's histogram and the scans' tile sums.
 */
#include "meshedges.hpp"

using namespace mlsgpu;

namespace
{

enum
{
    C_NON_FINITE = 0,           /* input coordinates */
    C_COLLAPSES = 1,            /* winners of all rounds */
    /* of one classification: cleared before each */
    C_EDGES = 2,
    C_INTERIOR = 3,
    C_FIXED = 4,
    C_USED = 5,                 /* vertices with a segment */
    C_SHORT = 6,
    C_BLOCKED = 7,
    C_CANDIDATES = 8,
    C_MIN_L2 = 9,               /* the bits of the smallest L2: a minimum, set to all ones before each */
    C_WORDS = 10,
    /* and a quality report's block (meshedges.hpp) before and after */
    ALL_WORDS = C_WORDS + 2 * Q_WORDS
};

const uint64_t NO_CANDIDATE = ~uint64_t(0);     /* a record's slot: a NaN's bits, which no L2 has */

/* the smallest 64-bit pattern of the wave, in every lane (a FULL wave) */
__device__ __forceinline__ uint64_t waveMin64(uint64_t bits) { return ~waveMax64(~bits); }

/* The sorted records of one classification with what the fixed kernel adds: the segment of x lists the participating
 * triangles that hold x -- record k is the side x -> to(k) of the triangle R.vals[k] / 3, whose third vertex is third[k]. */
struct Sides
{
    Records R;
    const uint2 *run;
    const uint32_t *third;
    const uint32_t *fixed;

    __device__ __forceinline__ uint32_t toOf(uint32_t k) const { return R.toOf(R.keys[k]); }
    __device__ __forceinline__ uint32_t valence(uint32_t x) const { return run[x].y - run[x].x; }
    __device__ __forceinline__ bool has(uint32_t from, uint32_t to) const { return sideOf(R, run, from, to) != (uint32_t) R.n; }
    /* body(v) for every vertex of S = {a, b} + N(a) + N(b), some of them more than once; stops when body returns false */
    template<typename Body>
    __device__ __forceinline__ bool forEachOfS(uint32_t a, uint32_t b, Body body) const
    {
        if (!body(a) || !body(b))
            return false;
        const uint32_t end[2] = {a, b};
        for (int e = 0; e < 2; e++)
        {
            const uint2 r = run[end[e]];
            for (uint32_t k = r.x; k < r.y; k++)
                if (!body(toOf(k)) || !body(third[k]))
                    return false;
        }
        return true;
    }
};

/* Step 5: which end survives, and where.  Not for an edge with both ends fixed. */
struct Survivor
{
    uint32_t survivor, removed;
    float position[3];
    __device__ __forceinline__ D3 at() const { return D3{(double) position[0], (double) position[1], (double) position[2]}; }
};
__device__ __forceinline__ Survivor survivorOf(const float *vertices, const uint32_t *fixed, uint32_t a, uint32_t b)
{
    const bool fa = fixed[a] != 0, fb = fixed[b] != 0;
    Survivor s;
    s.survivor = fb && !fa ? b : a;
    s.removed = fb && !fa ? a : b;
#pragma unroll
    for (int k = 0; k < 3; k++)
        s.position[k] = fa || fb ? vertices[3 * (uint64_t) s.survivor + k]
                                 : (float) (((double) vertices[3 * (uint64_t) a + k] + (double) vertices[3 * (uint64_t) b + k]) * 0.5);
    return s;
}

/* Step 2, and what the kernels behind it walk.  A record that is not alone in its run, or the head of a run without a reverse,
 * fixes both its ends; the first to set a vertex's flag counts it.  An edge is counted by its falling side, or by its rising
 * one where that finds no falling side.  A workgroup loops over the records in whole blocks and sends its three counts once
 * (fewer than 2^32 records: they fit 32 bits). */
__global__ __launch_bounds__(256) void fixedKernel(Records R, const uint2 *run, const uint32_t *tri, uint32_t *third, uint32_t *fixed,
                                                   Counter *counters)
{
    __shared__ GroupCounts<3> sums;
    sums.clear();
    const int at[3] = {C_EDGES, C_FIXED, C_USED};
    uint32_t count[3] = {0, 0, 0};
    const uint32_t n = (uint32_t) R.n;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < R.n; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        const uint64_t key = i < R.n ? R.keys[i] : R.dead();
        const uint64_t from = R.fromOf(key);
        if (from >= R.numVertices)
            continue;
        const uint32_t a = (uint32_t) from, b = R.toOf(key), s = R.vals[i];
        third[i] = tri[s - s % 3 + (s + 2) % 3];
        count[2] += R.segmentStart(i, from) ? 1u : 0u;
        const bool head = R.head(i, key);
        const bool open = head && sideOf(R, run, b, a) == n;
        count[0] += head && (a > b || open) ? 1u : 0u;
        if (open || !R.single(i, key))
        {
            count[1] += atomicOr(&fixed[a], 1u) == 0 ? 1u : 0u;
            count[1] += atomicOr(&fixed[b], 1u) == 0 ? 1u : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        sums.add(k, count[k]);
    sums.flush(counters, at);
}

/* Steps 3 to 6, and the first half of step 7.  The record at the head of a rising run speaks for its edge.  A workgroup loops
 * over the records in whole blocks, sends its four counts once and its smallest L2 once. */
__global__ __launch_bounds__(256) void classifyKernel(Sides S, const float *vertices, double limit, double minCos, uint64_t *slot,
                                                      Counter *bestLength, Counter *counters)
{
    __shared__ GroupCounts<4> sums;
    __shared__ Counter sLeast;
    if (threadIdx.x == 0)
        sLeast = NO_CANDIDATE;
    sums.clear();
    const int at[4] = {C_INTERIOR, C_SHORT, C_BLOCKED, C_CANDIDATES};
    uint32_t count[4] = {0, 0, 0, 0};
    uint64_t least = NO_CANDIDATE;
    const Records &R = S.R;
    const uint32_t n = (uint32_t) R.n;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < R.n; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        if (i >= R.n)
            continue;
        uint64_t mine = NO_CANDIDATE;
        const uint64_t key = R.keys[i];
        const uint32_t a = (uint32_t) R.fromOf(key), b = R.toOf(key);
        if (R.fromOf(key) < R.numVertices && a < b && R.single(i, key))
        {
            const uint32_t reverse = sideOf(R, S.run, b, a);
            const uint32_t c = S.third[i], d = reverse != n ? S.third[reverse] : c;
            if (reverse != n && R.single(reverse, R.keyOf(b, a)) && c != d)
            {
                count[0]++;
                const D3 pa = vertexAt(vertices, a), pb = vertexAt(vertices, b), e = pb - pa;
                const double L2 = dot(e, e);
                const uint64_t bits = (uint64_t) __double_as_longlong(L2);
                least = min(least, bits);
                if (L2 <= limit)
                {
                    count[1]++;
                    bool blocked = (S.fixed[a] != 0 && S.fixed[b] != 0) || S.valence(a) > MLSGPU_COLLAPSE_MAX_VALENCE
                                   || S.valence(b) > MLSGPU_COLLAPSE_MAX_VALENCE;        /* guards (i) and (ii) */
                    if (!blocked)
                    {
                        blocked = S.has(c, d) || S.has(d, c);   /* guard (iv) */
                        /* guard (iii): no vertex but c and d is a neighbour of both */
                        const uint2 ra = S.run[a];
                        for (uint32_t k = ra.x; k < ra.y && !blocked; k++)
                        {
                            const uint32_t other[2] = {S.toOf(k), S.third[k]};
                            for (int j = 0; j < 2; j++)
                                if (other[j] != b && other[j] != c && other[j] != d && (S.has(b, other[j]) || S.has(other[j], b)))
                                    blocked = true;
                        }
                    }
                    if (!blocked)
                    {
                        /* guard (v): no other triangle at a or b turns over or away */
                        const Survivor to = survivorOf(vertices, S.fixed, a, b);
                        const D3 pn = to.at();
                        const uint32_t t1 = R.vals[i] / 3, t2 = R.vals[reverse] / 3, end[2] = {a, b};
                        for (int e2 = 0; e2 < 2 && !blocked; e2++)
                        {
                            const uint2 r = S.run[end[e2]];
                            const D3 px = e2 == 0 ? pa : pb;
                            for (uint32_t k = r.x; k < r.y && !blocked; k++)
                            {
                                const uint32_t t = R.vals[k] / 3;
                                if (t == t1 || t == t2)
                                    continue;
                                const D3 pq = vertexAt(vertices, S.toOf(k)), pr = vertexAt(vertices, S.third[k]);
                                const D3 before = face(px, pq, pr), after = face(pn, pq, pr);
                                const double nn = dot(before, before), turn = dot(before, after);
                                if (nn != 0.0 && !(turn > 0.0 && turn >= (minCos * sqrt(nn)) * sqrt(dot(after, after))))
                                    blocked = true;
                            }
                        }
                    }
                    if (blocked)
                        count[2]++;
                    else
                    {
                        count[3]++;
                        mine = bits;
                        S.forEachOfS(a, b, [&](uint32_t v) {
                            if (bits < loadWord(&bestLength[v]))
                                atomicMin(&bestLength[v], (Counter) bits);
                            return true;
                        });
                    }
                }
            }
        }
        slot[i] = mine;
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
        sums.add(k, count[k]);
    const uint64_t ofWave = waveMin64(least);
    if (laneId() == 0 && ofWave != NO_CANDIDATE)
        atomicMin(&sLeast, (Counter) ofWave);
    sums.flush(counters, at);           /* (a barrier: sLeast is complete behind it) */
    if (threadIdx.x == 0 && sLeast != NO_CANDIDATE)
        atomicMin(&counters[C_MIN_L2], sLeast);
}

/* step 7, the tie: among the candidates that hold a vertex's best L2 the smallest key.  Few lanes get this far, and the word is
 * read first. */
__global__ __launch_bounds__(256) void keysKernel(Sides S, const uint64_t *slot, const Counter *bestLength, Counter *bestKey)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.R.n)
        return;
    const uint64_t bits = slot[i];
    if (bits == NO_CANDIDATE)
        return;
    const uint64_t key = S.R.keys[i];
    S.forEachOfS((uint32_t) S.R.fromOf(key), S.R.toOf(key), [&](uint32_t v) {
        if (bestLength[v] == bits && key < loadWord(&bestKey[v]))
            atomicMin(&bestKey[v], (Counter) key);
        return true;
    });
}

/* Steps 7 and 8.  A winner holds every vertex of its S, so no other winner's triangles touch its own, and it alone reads or
 * writes the rows and positions it names.  A workgroup loops over the records and sends its count once. */
__global__ __launch_bounds__(256) void applyKernel(Sides S, const uint64_t *slot, const Counter *bestLength, const Counter *bestKey,
                                                   float *vertices, uint32_t *tri, Counter *counters)
{
    __shared__ GroupCounts<1> sums;
    sums.clear();
    const int at[1] = {C_COLLAPSES};
    uint32_t winners = 0;
    const Records &R = S.R;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < R.n; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        const uint64_t bits = i < R.n ? slot[i] : NO_CANDIDATE;
        if (bits == NO_CANDIDATE)
            continue;
        const uint64_t key = R.keys[i];
        const uint32_t a = (uint32_t) R.fromOf(key), b = R.toOf(key);
        if (!S.forEachOfS(a, b, [&](uint32_t v) { return bestLength[v] == bits && bestKey[v] == key; }))
            continue;
        const Survivor to = survivorOf(vertices, S.fixed, a, b);
        const uint2 r = S.run[to.removed];
        for (uint32_t k = r.x; k < r.y; k++)
            tri[R.vals[k]] = to.survivor;
#pragma unroll
        for (int k = 0; k < 3; k++)
            vertices[3 * (uint64_t) to.survivor + k] = to.position[k];
        winners++;
    }
    sums.add(0, winners);
    sums.flush(counters, at);
}

/* Step 10: the flag stands at every vertex that has a segment in the last classification ... */
struct UsedIn
{
    const uint2 *run;
    __device__ __forceinline__ uint32_t operator()(uint64_t v) const { return run[v].y != 0 ? 1u : 0u; }
};
/* ... which gets its number and writes the bits it ended with */
struct VertexOut
{
    const uint32_t *vertices;   /* the positions as bits */
    uint32_t *number, *outVertices, *outSource;
    __device__ __forceinline__ void operator()(uint64_t v, uint32_t before, uint32_t flag) const
    {
        if (!flag)
            return;
        number[v] = before;
#pragma unroll
        for (int k = 0; k < 3; k++)
            outVertices[3 * (uint64_t) before + k] = vertices[3 * v + k];
        if (outSource != nullptr)
            outSource[before] = (uint32_t) v;
    }
};
/* and at every triangle that still takes part: its vertices have segments, so they have numbers */
struct LiveIn
{
    const uint32_t *tri;
    uint64_t numVertices;
    __device__ __forceinline__ uint32_t operator()(uint64_t t) const
    {
        const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
        return defectOf(i, numVertices).none() ? 1u : 0u;
    }
};
struct TriangleOut
{
    const uint32_t *tri, *number;
    uint32_t *outTriangles;
    __device__ __forceinline__ void operator()(uint64_t t, uint32_t before, uint32_t flag) const
    {
        if (!flag)
            return;
#pragma unroll
        for (int j = 0; j < 3; j++)
            outTriangles[3 * (uint64_t) before + j] = number[tri[3 * t + j]];
    }
};

double lengthOut(Counter bits)
{
    double d = INFINITY;
    if (bits != NO_CANDIDATE)
        std::memcpy(&d, &bits, sizeof(d));
    return d;
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_collapse_edges(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices,
                                              const uint32_t *dTriangles, uint64_t numTriangles, uint32_t maxRounds, double maxLength,
                                              double minCos, float *dOutVertices, uint64_t capVertices, uint32_t *dOutTriangles,
                                              uint64_t capTriangles, uint32_t *dOutSource, mlsgpu_collapse_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(maxLength) && maxLength >= 0.0 && minCos >= 0.0 && minCos <= 1.0, MLSGPU_ERR_INVALID);
    /* the sort's values and tile counts are 32-bit, and so are the indices of a triangle: 3 T < 2^32 */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || dVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->numVertices = numVertices;
    stats->numTriangles = numTriangles;
    stats->unusedVertices = numVertices;
    stats->minLengthSqBefore = stats->minLengthSqAfter = INFINITY;
    if ((numVertices == 0 || numTriangles == 0) && maxRounds > 0)
        stats->rounds = stats->converged = 1;   /* no triangle takes part: the first round finds no winner */
    if (numVertices == 0)
    {
        stats->outOfRangeTriangles = numTriangles;      /* every index is >= 0 vertices */
        return MLSGPU_OK;
    }

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t nv = numVertices, nt = numTriangles, n = 3 * nt;
    const double limit = maxLength * maxLength;
    const dim3 B(256);
    const SideKeys K = SideKeys::of(nv);
    DeviceArray<Counter> counters, best;
    DeviceArray<uint2> run;
    DeviceArray<uint32_t> third, fixed, number, tri, tileSums;
    DeviceArray<float> vertices;
    SortScratch sides;
    PROPAGATE(counters.alloc(ALL_WORDS));
    double scratch = (double) counters.bytes(ALL_WORDS);
    if (nt > 0)
    {
        const uint64_t tileElems = (uint64_t) scanTiles(std::max(nv, nt)) + 1;
        PROPAGATE(best.alloc(2 * nv));
        PROPAGATE(run.alloc(nv));
        PROPAGATE(fixed.alloc(nv));
        PROPAGATE(number.alloc(nv));
        PROPAGATE(vertices.alloc(3 * nv));
        PROPAGATE(third.alloc(n));
        PROPAGATE(tri.alloc(n));
        PROPAGATE(tileSums.alloc(tileElems));
        PROPAGATE(sides.alloc(n));
        scratch += (double) (best.bytes(2 * nv) + run.bytes(nv) + 2 * fixed.bytes(nv) + vertices.bytes(3 * nv) + 2 * third.bytes(n)
                             + tileSums.bytes(tileElems) + sides.bytes());
    }
    if (ctx->timing)
        ctx->addValue("collapse.scratch.bytes", scratch);
    Counter *const bestLength = best.get(), *const bestKey = best.get() + nv;
    Counter *const before = counters.get() + C_WORDS, *const after = before + Q_WORDS;

    Counter h[ALL_WORDS];
    HIP_CHECK(hipMemsetAsync(counters.get(), 0, sizeof(h), ctx->stream));
    LAUNCH(ctx, "kernel.collapse.check", checkKernel, dim3(divUp(nv, 256)), B, dVertices, nv, counters.get() + C_NON_FINITE);
    if (nt > 0)
    {
        HIP_CHECK(hipMemcpyAsync(vertices.get(), dVertices, nv * 12, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(tri.get(), dTriangles, nt * 12, hipMemcpyDeviceToDevice, ctx->stream));
        LAUNCH(ctx, "kernel.collapse.quality", qualityKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, (const float *) vertices.get(), nv,
               (const uint32_t *) tri.get(), nt, before);
    }
    /* step 9 */
    for (bool first = true; nt > 0; first = false)
    {
        HIP_CHECK(hipMemsetAsync(counters.get() + C_EDGES, 0, (C_MIN_L2 - C_EDGES) * sizeof(Counter), ctx->stream));
        HIP_CHECK(hipMemsetAsync(counters.get() + C_MIN_L2, 0xFF, sizeof(Counter), ctx->stream));
        HIP_CHECK(hipMemsetAsync(best.get(), 0xFF, 2 * nv * sizeof(Counter), ctx->stream));
        HIP_CHECK(hipMemsetAsync(run.get(), 0, nv * sizeof(uint2), ctx->stream));
        HIP_CHECK(hipMemsetAsync(fixed.get(), 0, nv * sizeof(uint32_t), ctx->stream));
        LAUNCH(ctx, "kernel.collapse.records", recordsKernel, dim3(divUp(nt, 256)), B, (const uint32_t *) tri.get(), nt, K, sides.keys());
        Records R;
        PROPAGATE(sides.sort(ctx, "kernel.collapse.sort", K, true, &R));
        uint64_t *const slot = sides.freeKeys();       /* the side of the sort that is free again */
        const Sides S{R, run.get(), third.get(), fixed.get()};
        const dim3 loop(std::min(divUp(n, 256), LOOP_BLOCKS));
        LAUNCH(ctx, "kernel.collapse.segments", segmentsKernel, dim3(divUp(n, 256)), B, R, run.get());
        LAUNCH(ctx, "kernel.collapse.fixed", fixedKernel, loop, B, R, (const uint2 *) run.get(), (const uint32_t *) tri.get(), third.get(),
               fixed.get(), counters.get());
        LAUNCH(ctx, "kernel.collapse.classify", classifyKernel, loop, B, S, (const float *) vertices.get(), limit, minCos, slot, bestLength,
               counters.get());
        HIP_CHECK(hipMemcpyAsync(h, counters.get(), C_WORDS * sizeof(Counter), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (h[C_NON_FINITE] != 0)
            break;
        if (first)
        {
            stats->numEdges = h[C_EDGES];
            stats->interiorEdges = h[C_INTERIOR];
            stats->fixedVertices = h[C_FIXED];
            stats->shortBefore = h[C_SHORT];
            stats->minLengthSqBefore = lengthOut(h[C_MIN_L2]);
        }
        stats->shortAfter = h[C_SHORT];
        stats->blockedAfter = h[C_BLOCKED];
        stats->minLengthSqAfter = lengthOut(h[C_MIN_L2]);
        stats->outVertices = h[C_USED];
        if (stats->rounds == maxRounds)
            break;
        stats->rounds++;
        if (h[C_CANDIDATES] == 0)       /* the best candidate of the mesh always wins: no candidate, no winner */
        {
            stats->converged = 1;
            break;
        }
        LAUNCH(ctx, "kernel.collapse.keys", keysKernel, dim3(divUp(n, 256)), B, S, (const uint64_t *) slot, (const Counter *) bestLength, bestKey);
        LAUNCH(ctx, "kernel.collapse.apply", applyKernel, loop, B, S, (const uint64_t *) slot, (const Counter *) bestLength,
               (const Counter *) bestKey, vertices.get(), tri.get(), counters.get());
    }
    if (nt > 0)
        LAUNCH(ctx, "kernel.collapse.quality", qualityKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, (const float *) vertices.get(), nv,
               (const uint32_t *) tri.get(), nt, after);
    HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h[C_NON_FINITE] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh collapse edges: %llu vertices have a coordinate that is not finite", h[C_NON_FINITE]);

    stats->collapses = h[C_COLLAPSES];
    stats->outOfRangeTriangles = h[C_WORDS + Q_OUT_OF_RANGE];
    stats->degenerateTriangles = h[C_WORDS + Q_DEGENERATE];
    qualityOut(h + C_WORDS, &stats->minQualityBefore, stats->qualityBefore);
    qualityOut(h + C_WORDS + Q_WORDS, &stats->minQualityAfter, stats->qualityAfter);
    for (int k = 0; k < 16; k++)
        stats->outTriangles += stats->qualityAfter[k];  /* every triangle that still takes part is in one bin */
    stats->unusedVertices = nv - stats->outVertices;
    if (capVertices < stats->outVertices || capTriangles < stats->outTriangles)
        return setError(MLSGPU_ERR_LENGTH, "mesh collapse edges: the outputs hold %llu vertices and %llu triangles, the result has %llu and %llu",
                        (unsigned long long) capVertices, (unsigned long long) capTriangles, (unsigned long long) stats->outVertices,
                        (unsigned long long) stats->outTriangles);
    REQUIRE(stats->outVertices == 0 || dOutVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(stats->outTriangles == 0 || dOutTriangles != nullptr, MLSGPU_ERR_INVALID);

    if (stats->outTriangles > 0)        /* then there are vertices too */
    {
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.collapse.vertices", UsedIn{run.get()},
                                           VertexOut{reinterpret_cast<const uint32_t *>(vertices.get()), number.get(),
                                                     reinterpret_cast<uint32_t *>(dOutVertices), dOutSource},
                                           nv, 0u, tileSums.get(), (uint32_t *) nullptr)));
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.collapse.triangles", LiveIn{tri.get(), nv},
                                           TriangleOut{tri.get(), number.get(), dOutTriangles}, nt, 0u, tileSums.get(),
                                           (uint32_t *) nullptr)));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));   /* the scratch goes with the call */
    }
    return MLSGPU_OK;
}
