/*
 * Long-edge split of an indexed triangle mesh that is resident in HBM, with a triangle quality report: the refine step next to
 * collapse.hip, flip.hip and smooth.hip.  The reference has no counterpart.  The contract (include/mlsgpu_hip.h, DESIGN.md
 * "Mesh edge split") is Rivara's longest-edge bisection, written so that a round needs no arbitration: an edge is split only
 * where it is the first side of every triangle that holds it, so two splits of a round never share a triangle, and every
 * output is a count, a maximum or something that one thread writes.
 *
 *   check      a thread per vertex: the coordinates that are not finite                                  } meshedges.hpp
 *   quality    over the triangles, before the first round and after the last: classes, histogram, the smallest q
 *   work       a thread per input row: the working copy, with the rows that take no part made dead for every round
 *   per classification:
 *     edges    a thread per row: its three sides as keys lo << b | hi, b the bit length of the round's V (dead ones for a row
 *              that takes no part); the sort numbers them, so a record's value is 3 * row + corner
 *     sort     the keys: the sides of one edge, whichever way they run, become one run, and the runs stand in ascending (a, b)
 *     classify over the records, at the head of a run: one record is a boundary edge, two that run opposite ways an interior
 *              one (the row says which way a side runs), anything else is irregular; L2, the pins, and for a splittable long
 *              edge the other two sides of its one or two triangles; the rows its split adds (0, 1 or 2) and the values of
 *              its two sides go to the record's slots
 *                                                                                     } one read-back: the counts
 *   per round:
 *     rewrite  one scan over the records' rows-to-add: a candidate learns its number j and its offset o_j (the heads stand in
 *              ascending (a, b)) and writes its vertex, its ends, the corner b of its rows and its new rows
 *   at the end:
 *     rows     a thread per output row: the working row, or the input's where that took no part
 *
 * The collapse and the flips sort DIRECTED sides and search a side's reverse in its vertex's segment (meshedges.hpp).  Here
 * the two sides of an edge are neighbours in the sorted records: nothing is searched, no segments are built, and -- what
 * step 7 needs -- a boundary edge whose only side runs b -> a stands where (a, b) belongs, not where (b, a) does.
 *
 * classify writes no row and no position.  rewrite reads the positions of its own a and b and the third corners of its own
 * triangles, and writes the corner b of those triangles, rows behind T_r and a position behind V_r that are its own: no
 * kernel races with itself.  An index >= V is compared and counted, never used as an address.
 *
 * The mesh grows.  The read-back of a classification tells the host how many vertices and rows the round adds before it
 * rewrites: there the limit of step 8 is checked, and the working arrays grow to at least twice their size by a
 * device-to-device copy.  The sort's scratch and the scan's tile sums hold nothing between two rounds and are simply
 * allocated again.  Scratch belongs to the call (the header lists it).
 */
#include "meshedges.hpp"

using namespace mlsgpu;

namespace
{

enum
{
    C_NON_FINITE = 0,           /* input coordinates */
    /* of one classification: cleared before each */
    C_EDGES = 1,
    C_INTERIOR = 2,
    C_BOUNDARY = 3,
    C_LONG = 4,
    C_BLOCKED = 5,
    C_CANDIDATES = 6,
    C_BOUNDARY_CANDIDATES = 7,
    C_MAX_L2 = 8,               /* the bits of the largest L2: a maximum from 0 */
    C_WORDS = 9,
    /* and a quality report's block (meshedges.hpp) before and after */
    ALL_WORDS = C_WORDS + 2 * Q_WORDS
};

const uint32_t DEAD_INDEX = 0xFFFFFFFFu;        /* V < 2^32 in every round: an index no round has */

/* Step 1 is decided on the input.  A row that takes no part must not come to life when V grows past one of its indices: its
 * working copy is dead for every V, and rowsKernel hands the input's bits back. */
__global__ __launch_bounds__(256) void workKernel(const uint32_t *tri, uint64_t numTriangles, uint64_t numVertices, uint32_t *work)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    const bool live = defectOf(i, numVertices).none();
#pragma unroll
    for (int k = 0; k < 3; k++)
        work[3 * t + k] = live ? (uint32_t) i[k] : DEAD_INDEX;
}

/* Step 9: rows 0 .. T - 1 in their places, the new rows behind them. */
__global__ __launch_bounds__(256) void rowsKernel(const uint32_t *work, uint64_t outTriangles, const uint32_t *tri, uint64_t numTriangles,
                                                  uint64_t numVertices, uint32_t *out)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= outTriangles)
        return;
    bool live = true;
    uint64_t i[3] = {0, 0, 0};
    if (t < numTriangles)
    {
#pragma unroll
        for (int k = 0; k < 3; k++)
            i[k] = tri[3 * t + k];
        live = defectOf(i, numVertices).none();
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        out[3 * t + k] = live ? work[3 * t + k] : (uint32_t) i[k];
}

/* the three sides of a row as undirected keys; three dead records for a row that takes no part */
__global__ __launch_bounds__(256) void edgesKernel(const uint32_t *tri, uint64_t numTriangles, SideKeys K, uint64_t *keys)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    const bool live = defectOf(i, K.numVertices).none();
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const uint64_t x = i[k], y = i[k == 2 ? 0 : k + 1];
        keys[3 * t + k] = live ? K.keyOf(min(x, y), max(x, y)) : K.dead();
    }
}

const uint32_t NO_SIDE = 0xFFFFFFFFu;           /* 3 T < 2^32: no record has this value */

/* step 3: the same bits whichever end comes first */
__device__ __forceinline__ double lengthSq(const D3 &p, const D3 &q)
{
    const D3 e = q - p;
    return dot(e, e);
}

/* the third vertex of the triangle of a record whose value is s = 3 * row + the corner its side leaves */
__device__ __forceinline__ uint32_t thirdOf(const uint32_t *tri, uint32_t s) { return tri[s - s % 3 + (s + 2) % 3]; }

/* Step 5 for the edge a < b in the triangle whose third vertex is x: it comes before both other sides. */
__device__ __forceinline__ bool firstSide(const float *vertices, double L2, uint32_t a, uint32_t b, const D3 &pa, const D3 &pb, uint32_t x)
{
    const D3 px = vertexAt(vertices, x);
    const double ofA = lengthSq(pa, px), ofB = lengthSq(pb, px);
    /* against {a, x}: equal lo or a smaller one decides by hi; against {b, x}: a < b is min(b, x) unless x < a */
    const bool beforeA = L2 > ofA || (L2 == ofA && (x < a ? false : b < x));
    const bool beforeB = L2 > ofB || (L2 == ofB && a < x);
    return beforeA && beforeB;
}

/* Steps 2 to 6.  A workgroup loops over the records in whole blocks, sends its seven counts once and its largest L2 once
 * (fewer than 2^32 records: the counts fit 32 bits).  sides[i] of a candidate: the values of its side a -> b (high word) and
 * of its side b -> a (low word), NO_SIDE where it has none. */
__global__ __launch_bounds__(256) void classifyKernel(Records R, const float *vertices, const uint32_t *tri, const uint8_t *pinned,
                                                      uint32_t numPinned, double limit, uint32_t *rows, uint64_t *sides, Counter *counters)
{
    __shared__ GroupCounts<7> sums;
    __shared__ Counter sMost;
    if (threadIdx.x == 0)
        sMost = 0;
    sums.clear();
    const int at[7] = {C_EDGES, C_INTERIOR, C_BOUNDARY, C_LONG, C_BLOCKED, C_CANDIDATES, C_BOUNDARY_CANDIDATES};
    uint32_t count[7] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t most = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < R.n; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        if (i >= R.n)
            continue;
        uint32_t mine = 0, rising = NO_SIDE, falling = NO_SIDE;
        const uint64_t key = R.keys[i];
        if (R.fromOf(key) < R.numVertices && R.head(i, key))
        {
            const uint32_t a = (uint32_t) R.fromOf(key), b = R.toOf(key);
            const uint32_t uses = i + 1 < R.n && R.keys[i + 1] == key ? (i + 2 < R.n && R.keys[i + 2] == key ? 3u : 2u) : 1u;
            /* a side's value is 3 * row + the corner it leaves: the row says which way it runs */
            const uint32_t s0 = R.vals[i], s1 = uses == 2 ? R.vals[i + 1] : NO_SIDE;
            const bool up0 = tri[s0] == a, up1 = s1 != NO_SIDE && tri[s1] == a;
            const uint32_t x0 = thirdOf(tri, s0), x1 = s1 != NO_SIDE ? thirdOf(tri, s1) : x0;
            const bool boundary = uses == 1;
            const bool interior = uses == 2 && up0 != up1 && x0 != x1;
            count[0]++;
            count[1] += interior ? 1u : 0u;
            count[2] += boundary ? 1u : 0u;
            const D3 pa = vertexAt(vertices, a), pb = vertexAt(vertices, b);
            const double L2 = lengthSq(pa, pb);
            most = max(most, (uint64_t) __double_as_longlong(L2));
            if (L2 > limit)
            {
                count[3]++;
                const bool bothPinned = pinned != nullptr && a < numPinned && b < numPinned && pinned[a] != 0 && pinned[b] != 0;
                if (!(interior || boundary) || bothPinned)
                    count[4]++;
                else if (firstSide(vertices, L2, a, b, pa, pb, x0) && (!interior || firstSide(vertices, L2, a, b, pa, pb, x1)))
                {
                    mine = interior ? 2u : 1u;
                    rising = up0 ? s0 : up1 ? s1 : NO_SIDE;
                    falling = !up0 ? s0 : interior ? s1 : NO_SIDE;
                    count[5]++;
                    count[6] += boundary ? 1u : 0u;
                }
            }
        }
        rows[i] = mine;
        sides[i] = (uint64_t) rising << 32 | falling;
    }
#pragma unroll
    for (int k = 0; k < 7; k++)
        sums.add(k, count[k]);
    const uint64_t ofWave = waveMax64(most);
    if (laneId() == 0 && ofWave != 0)
        atomicMax(&sMost, (Counter) ofWave);
    sums.flush(counters, at);           /* (a barrier: sMost is complete behind it) */
    if (threadIdx.x == 0 && sMost != 0)
        atomicMax(&counters[C_MAX_L2], sMost);
}

/* Step 7.  What the scan adds up per record: a candidate's one vertex and its one or two rows ... */
struct Added
{
    const uint32_t *rows;
    __device__ __forceinline__ U3 operator()(uint64_t i) const
    {
        const uint32_t r = rows[i];
        return U3{r != 0 ? 1u : 0u, r, 0u};
    }
};
/* ... and what a candidate does with its j and o_j */
struct Rewrite
{
    Records R;
    const uint64_t *sides;
    float *vertices;
    uint32_t *tri, *ends;
    uint32_t inVertices, roundVertices, roundTriangles;        /* V, V_r, T_r */

    __device__ __forceinline__ void operator()(uint64_t i, U3 before, U3 value) const
    {
        if (value.a == 0)
            return;
        const uint64_t key = R.keys[i];
        const uint32_t a = (uint32_t) R.fromOf(key), b = R.toOf(key), m = roundVertices + before.a;
        const uint32_t rising = (uint32_t) (sides[i] >> 32), falling = (uint32_t) sides[i];
        uint64_t row = roundTriangles + before.b;
        if (rising != NO_SIDE)          /* T1: a at the side's corner, b behind it */
        {
            const uint32_t s = rising, c = thirdOf(tri, s);
            tri[s - s % 3 + (s + 1) % 3] = m;
            tri[3 * row] = m;
            tri[3 * row + 1] = b;
            tri[3 * row + 2] = c;
            row++;
        }
        if (falling != NO_SIDE)         /* T2: b at the side's corner */
        {
            const uint32_t s = falling, d = thirdOf(tri, s);
            tri[s] = m;
            tri[3 * row] = b;
            tri[3 * row + 1] = m;
            tri[3 * row + 2] = d;
        }
#pragma unroll
        for (int k = 0; k < 3; k++)
            vertices[3 * (uint64_t) m + k] = (float) (((double) vertices[3 * (uint64_t) a + k] + (double) vertices[3 * (uint64_t) b + k]) * 0.5);
        ends[2 * (uint64_t) (m - inVertices)] = a;
        ends[2 * (uint64_t) (m - inVertices) + 1] = b;
    }
};

double lengthOut(Counter bits)
{
    double d;
    std::memcpy(&d, &bits, sizeof(d));
    return d;
}

/* `array` with room for `room` elements, the first `used` of them kept: what a growing mesh needs of its working arrays */
template<typename T>
int grow(mlsgpu_ctx *ctx, DeviceArray<T> &array, uint64_t used, uint64_t room)
{
    DeviceArray<T> larger;
    PROPAGATE(larger.alloc(room));
    if (used > 0)
        HIP_CHECK(hipMemcpyAsync(larger.get(), array.get(), used * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));       /* the old array goes here */
    array = std::move(larger);
    return MLSGPU_OK;
}

const uint64_t VERTEX_LIMIT = uint64_t(1) << 32;                /* outVertices < 2^32 */
const uint64_t TRIANGLE_LIMIT = ((uint64_t(1) << 32) + 2) / 3;  /* 3 * outTriangles < 2^32 */

int sizeError(uint64_t capVertices, uint64_t capTriangles, const mlsgpu_split_stats *stats)
{
    return setError(MLSGPU_ERR_LENGTH, "mesh split edges: the outputs hold %llu vertices and %llu triangles, the result has %llu and %llu",
                    (unsigned long long) capVertices, (unsigned long long) capTriangles, (unsigned long long) stats->outVertices,
                    (unsigned long long) stats->outTriangles);
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_split_edges(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                           uint64_t numTriangles, uint32_t maxRounds, double maxLength, uint64_t maxOutTriangles,
                                           const uint8_t *dPinned, float *dOutVertices, uint64_t capVertices, uint32_t *dOutTriangles,
                                           uint64_t capTriangles, uint32_t *dOutEnds, mlsgpu_split_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(maxLength) && maxLength > 0.0 && (maxOutTriangles == 0 || maxOutTriangles >= numTriangles), MLSGPU_ERR_INVALID);
    /* the sort's values and tile counts are 32-bit, and so are the indices of a triangle: 3 T < 2^32 */
    REQUIRE(numVertices < VERTEX_LIMIT && numTriangles < TRIANGLE_LIMIT, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || dVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->numVertices = stats->outVertices = numVertices;
    stats->numTriangles = stats->outTriangles = numTriangles;
    if ((numVertices == 0 || numTriangles == 0) && maxRounds > 0)
        stats->rounds = stats->converged = 1;   /* no triangle takes part: the first round finds no candidate */
    if (numVertices == 0 && numTriangles == 0)
        return MLSGPU_OK;

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t nv = numVertices, nt = numTriangles;
    const dim3 B(256);
    if (nv == 0)
    {
        stats->outOfRangeTriangles = nt;        /* every index is >= 0 vertices: the rows keep their bits */
        if (capTriangles < nt)
            return sizeError(capVertices, capTriangles, stats);
        REQUIRE(dOutTriangles != nullptr, MLSGPU_ERR_INVALID);
        HIP_CHECK(hipMemcpyAsync(dOutTriangles, dTriangles, nt * 12, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MLSGPU_OK;
    }

    const double limit = maxLength * maxLength;
    DeviceArray<Counter> counters;
    DeviceArray<uint32_t> tri, ends;
    DeviceArray<U3> tileSums;
    DeviceArray<float> vertices;
    SortScratch sides;
    /* the mesh as the rounds leave it, and the room of its working arrays */
    uint64_t curV = nv, curT = nt, roomV = nv, roomT = nt;
    PROPAGATE(counters.alloc(ALL_WORDS));
    if (nt > 0)
    {
        PROPAGATE(vertices.alloc(3 * roomV));
        PROPAGATE(tri.alloc(3 * roomT));
    }
    Counter *const before = counters.get() + C_WORDS, *const after = before + Q_WORDS;

    Counter h[ALL_WORDS];
    HIP_CHECK(hipMemsetAsync(counters.get(), 0, sizeof(h), ctx->stream));
    LAUNCH(ctx, "kernel.split.check", checkKernel, dim3(divUp(nv, 256)), B, dVertices, nv, counters.get() + C_NON_FINITE);
    if (nt > 0)
    {
        HIP_CHECK(hipMemcpyAsync(vertices.get(), dVertices, nv * 12, hipMemcpyDeviceToDevice, ctx->stream));
        LAUNCH(ctx, "kernel.split.work", workKernel, dim3(divUp(nt, 256)), B, dTriangles, nt, nv, tri.get());
        LAUNCH(ctx, "kernel.split.quality", qualityKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, dVertices, nv, dTriangles, nt, before);
    }
    /* step 8 */
    for (bool first = true; nt > 0; first = false)
    {
        /* what holds nothing between two rounds follows the mesh's room */
        const uint64_t n = 3 * curT, tileElems = (uint64_t) scanTiles(3 * roomT) + 1;
        if (sides.keysA.capacity() < 3 * roomT)
        {
            PROPAGATE(sides.alloc(3 * roomT));
            PROPAGATE(tileSums.alloc(tileElems));
        }
        sides.n = n;            /* the records of this round: the first n of the room */
        const SideKeys K = SideKeys::of(curV);
        HIP_CHECK(hipMemsetAsync(counters.get() + C_EDGES, 0, (C_WORDS - C_EDGES) * sizeof(Counter), ctx->stream));
        LAUNCH(ctx, "kernel.split.edges", edgesKernel, dim3(divUp(curT, 256)), B, (const uint32_t *) tri.get(), curT, K, sides.keys());
        Records R;
        PROPAGATE(sides.sort(ctx, "kernel.split.sort", K, true, &R));
        /* the side of the sort that is free again: a 64-bit and a 32-bit word per record */
        uint64_t *const ofEdge = sides.freeKeys();
        uint32_t *const rows = sides.freeVals();
        LAUNCH(ctx, "kernel.split.classify", classifyKernel, dim3(std::min(divUp(n, 256), LOOP_BLOCKS)), B, R, (const float *) vertices.get(),
               (const uint32_t *) tri.get(), dPinned, (uint32_t) nv, limit, rows, ofEdge, counters.get());
        HIP_CHECK(hipMemcpyAsync(h, counters.get(), C_WORDS * sizeof(Counter), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (h[C_NON_FINITE] != 0)
            break;
        if (first)
        {
            stats->numEdges = h[C_EDGES];
            stats->interiorEdges = h[C_INTERIOR];
            stats->boundaryEdges = h[C_BOUNDARY];
            stats->longBefore = h[C_LONG];
            stats->maxLengthSqBefore = lengthOut(h[C_MAX_L2]);
        }
        stats->longAfter = h[C_LONG];
        stats->blockedAfter = h[C_BLOCKED];
        stats->maxLengthSqAfter = lengthOut(h[C_MAX_L2]);
        if (stats->rounds == maxRounds)
            break;
        if (h[C_CANDIDATES] == 0)       /* the longest splittable edge that is first in its triangles always is one */
        {
            stats->rounds++;
            stats->converged = 1;
            break;
        }
        /* a round is all or nothing: the limit is checked where its size is known */
        const uint64_t nextV = curV + h[C_CANDIDATES], nextT = curT + 2 * h[C_CANDIDATES] - h[C_BOUNDARY_CANDIDATES];
        if ((maxOutTriangles != 0 && nextT > maxOutTriangles) || nextV >= VERTEX_LIMIT || nextT >= TRIANGLE_LIMIT)
        {
            stats->limited = 1;
            break;
        }
        stats->rounds++;
        stats->splits += h[C_CANDIDATES];
        stats->boundarySplits += h[C_BOUNDARY_CANDIDATES];
        if (nextV > roomV)
        {
            const uint64_t room = std::min(std::max(nextV, 2 * roomV), VERTEX_LIMIT - 1);
            PROPAGATE(grow(ctx, vertices, 3 * curV, 3 * room));
            PROPAGATE(grow(ctx, ends, 2 * (curV - nv), 2 * (room - nv)));
            roomV = room;
        }
        if (nextT > roomT)
        {
            const uint64_t room = std::min(std::max(nextT, 2 * roomT), TRIANGLE_LIMIT - 1);
            PROPAGATE(grow(ctx, tri, 3 * curT, 3 * room));
            roomT = room;
        }
        PROPAGATE((exclusiveScan<U3>(ctx, "kernel.split.rewrite", Added{rows},
                                     Rewrite{R, (const uint64_t *) ofEdge, vertices.get(), tri.get(), ends.get(), (uint32_t) nv, (uint32_t) curV, (uint32_t) curT},
                                     n, U3{0u, 0u, 0u}, tileSums.get(), (U3 *) nullptr)));
        curV = nextV;
        curT = nextT;
    }
    if (nt > 0)
        LAUNCH(ctx, "kernel.split.quality", qualityKernel, dim3(std::min(divUp(curT, 256), LOOP_BLOCKS)), B, (const float *) vertices.get(), curV,
               (const uint32_t *) tri.get(), curT, after);
    HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h[C_NON_FINITE] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh split edges: %llu vertices have a coordinate that is not finite", h[C_NON_FINITE]);
    sides.n = sides.keysA.capacity();           /* what was allocated, not the last round's records */
    if (ctx->timing)
        ctx->addValue("split.scratch.bytes",
                      (double) (counters.bytes(ALL_WORDS) + vertices.bytes(3 * roomV) + tri.bytes(3 * roomT) + ends.bytes(2 * (roomV - nv))
                                + tileSums.bytes(tileSums.capacity()) + (nt > 0 ? sides.bytes() : 0)));

    stats->outOfRangeTriangles = h[C_WORDS + Q_OUT_OF_RANGE];
    stats->degenerateTriangles = h[C_WORDS + Q_DEGENERATE];
    qualityOut(h + C_WORDS, &stats->minQualityBefore, stats->qualityBefore);
    qualityOut(h + C_WORDS + Q_WORDS, &stats->minQualityAfter, stats->qualityAfter);
    stats->outVertices = curV;
    stats->outTriangles = curT;
    if (capVertices < stats->outVertices || capTriangles < stats->outTriangles)
        return sizeError(capVertices, capTriangles, stats);
    REQUIRE(dOutVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(stats->outTriangles == 0 || dOutTriangles != nullptr, MLSGPU_ERR_INVALID);

    HIP_CHECK(hipMemcpyAsync(dOutVertices, nt > 0 ? vertices.get() : dVertices, curV * 12, hipMemcpyDeviceToDevice, ctx->stream));
    if (curT > 0)
        LAUNCH(ctx, "kernel.split.rows", rowsKernel, dim3(divUp(curT, 256)), B, (const uint32_t *) tri.get(), curT, dTriangles, nt, nv, dOutTriangles);
    if (dOutEnds != nullptr && curV > nv)
        HIP_CHECK(hipMemcpyAsync(dOutEnds, ends.get(), (curV - nv) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));       /* the scratch goes with the call */
    return MLSGPU_OK;
}
