/*
 * Taubin lambda|mu smoothing of an indexed triangle mesh that is resident in HBM.  The reference has no counterpart: its
 * meshes leave the device as marching made them.  The contract (include/mlsgpu_hip.h, DESIGN.md "Mesh smoothing") is written
 * so that every output is an integer sum or one correctly rounded operation away from one: the result depends neither on
 * the schedule nor on how the triangles are ordered, and renumbering the vertices permutes it.
 *
 *   load       a thread per vertex: the packed rows into 16-byte working rows, the largest |coordinate| (an atomicMax on the
 *              bits of the float, one per wave), the coordinates that are not finite
 *   records    a thread per triangle: its class, and both directions of its three sides as keys from << b | to
 *   sort       the keys: the records that leave a vertex become one segment, equal records one run; the length of the run of
 *              (a, b) is how many triangle sides use the edge {a, b}, in either direction
 *   mark       over the records: edges, boundary edges (a run of one), the vertices on them, the vertices with a segment
 *   adjacency  a scan over the run heads that step 3 of the contract keeps: the neighbour lists, and where each vertex's starts
 *              and ends                                                                                  } one read-back:
 *   pass       a thread per vertex, once per pass: gathers its run from one working array into the other } the extent sizes
 *   finish     over the vertices: the packed rows out, the largest move, the boundary vertices           } the fixed point
 *
 * An index >= V is compared and counted, never used as an address; no address depends on a coordinate.
 *
 * Scratch belongs to the call: 144 bytes per triangle (six records: the two sides of the sort's keys 96 and values 48; the
 * neighbour lists lie in the key side the sort leaves free), 41 bytes per vertex (two working arrays 32, neighbour run 8,
 * boundary flag 1), the sort's histogram (4 KB per 4096 records) and the scan's tile sums.
 */
#include "meshpost.hpp"

#include <cmath>
#include <cstdlib>

using namespace mlsgpu;

namespace
{

enum
{
    C_OUT_OF_RANGE = 0,
    C_DEGENERATE = 1,
    C_EDGES = 2,
    C_BOUNDARY_EDGES = 3,
    C_USED_VERTICES = 4,        /* vertices with a segment: the others are isolated */
    C_BOUNDARY_VERTICES = 5,
    C_NON_FINITE = 6,           /* input coordinates */
    C_INPUT_MAX = 7,            /* the bits of the largest |coordinate| of the input */
    C_PASS_MAX = 8,             /* ... of the passes' outputs */
    C_MAX_MOVE = 9,             /* the bits of the largest move, a double */
    C_WORDS = 10
};

__device__ __forceinline__ uint32_t absBits(float x) { return __float_as_uint(fabsf(x)); }

/* Every lane of every wave stays to the end: foldMax needs the full wave. */
__global__ __launch_bounds__(256) void loadKernel(const float *vertices, uint64_t numVertices, float4 *work, Counter *counters)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < numVertices;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live)
    {
        p.x = vertices[3 * v];
        p.y = vertices[3 * v + 1];
        p.z = vertices[3 * v + 2];
        work[v] = p;
    }
    tally(!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z)), &counters[C_NON_FINITE]);
    foldMax(max(max(absBits(p.x), absBits(p.y)), absBits(p.z)), &counters[C_INPUT_MAX]);
}

/* steps 1 and 2 of the contract: both directions of a triangle's three sides; six dead records for one that takes no part */
__global__ __launch_bounds__(256) void recordsKernel(const uint32_t *tri, uint64_t numTriangles, SideKeys K, uint64_t *keys,
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
    {
        const uint64_t from = i[k], to = i[k == 2 ? 0 : k + 1];
        keys[6 * t + 2 * k] = d.none() ? K.keyOf(from, to) : K.dead();
        keys[6 * t + 2 * k + 1] = d.none() ? K.keyOf(to, from) : K.dead();
    }
}

/* step 2.  Both directions of every side are there, so a run of one is an edge that exactly one triangle side uses, and each
 * end of such a boundary edge is marked by the record that leaves it; an edge is counted by the direction that rises.  The
 * plain byte stores race only with stores of the same value.  A workgroup loops over the records (at most 2^32 / LOOP_BLOCKS
 * of them: its counts fit 32 bits) and sends its three counts once. */
__global__ __launch_bounds__(256) void markKernel(Records R, uint8_t *onBoundary, Counter *counters)
{
    __shared__ GroupCounts<3> sums;
    sums.clear();
    const int at[3] = {C_EDGES, C_BOUNDARY_EDGES, C_USED_VERTICES};
    uint32_t count[3] = {0, 0, 0};
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < R.n; i += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t key = R.keys[i], from = R.fromOf(key);
        if (from >= R.numVertices)
            continue;           /* the record of a triangle that takes no part */
        const bool rises = from < R.toOf(key);
        const bool single = R.single(i, key);
        if (single)
            onBoundary[from] = 1;
        count[0] += rises && R.head(i, key) ? 1u : 0u;
        count[1] += rises && single ? 1u : 0u;
        count[2] += R.segmentStart(i, from) ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
        sums.add(k, count[k]);
    sums.flush(counters, at);
}

/* step 3: the heads of the runs that stay in the neighbour lists */
struct KeepIn
{
    Records R;
    const uint8_t *onBoundary;
    bool curve;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        const uint64_t key = R.keys[i], from = R.fromOf(key);
        if (from >= R.numVertices || !R.head(i, key))
            return 0u;
        if (!onBoundary[from])
            return 1u;
        return curve && R.single(i, key) ? 1u : 0u;
    }
};
/* run[v] = where the list of v starts and ends: written by the first and by the last record of v's segment (a vertex without
 * a segment keeps the zeros it was cleared to) */
struct ListOut
{
    Records R;
    uint32_t *neighbours;
    uint2 *run;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t before, uint32_t kept) const
    {
        const uint64_t key = R.keys[i], from = R.fromOf(key);
        if (from >= R.numVertices)
            return;
        if (kept)
            neighbours[before] = R.toOf(key);
        if (R.segmentStart(i, from))
            run[from].x = before;
        if (R.segmentEnd(i, from))
            run[from].y = before + kept;
    }
};

/* Step 5, with meshpost.hpp's quantise as Q (a call that has not diverged stays below 2^52; one that has meets the clamp).
 * One aligned 16-byte load per neighbour; the sums are unsigned, so that they wrap.  Every lane stays to the end.
 * BATCHED: four neighbours a round, their four index loads issued together and then their four rows, so that a list costs a
 * quarter of the dependent round trips (a slot past the end reads the list's last entry again and adds nothing); otherwise
 * one neighbour after the other.  The sums are integers: the same bits either way. */
template<bool BATCHED>
__global__ __launch_bounds__(256) void passKernel(const float4 *in, float4 *out, const uint2 *run, const uint32_t *neighbours,
                                                  uint64_t numVertices, double scale, double invScale, double F, Counter *counters)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < numVertices;
    float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live)
    {
        p = in[v];
        const uint2 r = run[v];
        const uint32_t k = r.y - r.x;
        if (k > 0)
        {
            unsigned long long S[3] = {0, 0, 0};
            if (BATCHED)
                for (uint32_t j = r.x; j < r.y; j += 4)
                {
                    bool has[4];
                    uint32_t n[4];
                    float4 q[4];
#pragma unroll
                    for (int i = 0; i < 4; i++)
                    {
                        has[i] = j + i < r.y;
                        n[i] = neighbours[min(j + i, r.y - 1)];
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        q[i] = in[n[i]];
#pragma unroll
                    for (int i = 0; i < 4; i++)
                    {
                        S[0] += has[i] ? (unsigned long long) quantise(q[i].x, scale) : 0ull;
                        S[1] += has[i] ? (unsigned long long) quantise(q[i].y, scale) : 0ull;
                        S[2] += has[i] ? (unsigned long long) quantise(q[i].z, scale) : 0ull;
                    }
                }
            else
                for (uint32_t j = r.x; j < r.y; j++)
                {
                    const float4 q = in[neighbours[j]];
                    S[0] += (unsigned long long) quantise(q.x, scale);
                    S[1] += (unsigned long long) quantise(q.y, scale);
                    S[2] += (unsigned long long) quantise(q.z, scale);
                }
            const float own[3] = {p.x, p.y, p.z};
            float moved[3];
#pragma unroll
            for (int a = 0; a < 3; a++)
            {
                const long long D = (long long) (S[a] - (unsigned long long) k * (unsigned long long) quantise(own[a], scale));
                const double d = ((double) D / (double) k) * invScale;
                moved[a] = (float) ((double) own[a] + F * d);
            }
            p = make_float4(moved[0], moved[1], moved[2], 0.0f);
        }
        out[v] = p;
    }
    foldMax(max(max(absBits(p.x), absBits(p.y)), absBits(p.z)), &counters[C_PASS_MAX]);
}

/* Step 7 and the way out.  A thread reads its input row before it writes its output row: the two may be the same.  A workgroup
 * loops over the vertices and sends its count and its maximum once. */
__global__ __launch_bounds__(256) void finishKernel(const float *vertices, const float4 *work, const uint8_t *onBoundary,
                                                    uint64_t numVertices, float *outVertices, Counter *counters)
{
    __shared__ GroupCounts<1> sBoundary;
    __shared__ Counter sMove;
    if (threadIdx.x == 0)
        sMove = 0;
    sBoundary.clear();
    const int at[1] = {C_BOUNDARY_VERTICES};
    uint32_t boundary = 0;
    uint64_t bits = 0;          /* of the largest move, a double */
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < numVertices; v += (uint64_t) gridDim.x * blockDim.x)
    {
        const float was[3] = {vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]};
        const float4 p = work[v];
        const float is[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int a = 0; a < 3; a++)
        {
            bits = max(bits, (uint64_t) __double_as_longlong(fabs((double) is[a] - (double) was[a])));
            outVertices[3 * v + a] = is[a];
        }
        boundary += onBoundary[v] != 0 ? 1u : 0u;
    }
    sBoundary.add(0, boundary);
    const uint64_t most = waveMax64(bits);
    if (laneId() == 0)
        atomicMax(&sMove, (Counter) most);
    sBoundary.flush(counters, at);      /* (a barrier: sMove is complete behind it) */
    if (threadIdx.x == 0 && sMove != 0)
        atomicMax(&counters[C_MAX_MOVE], sMove);
}

/* MLSGPU_HIP_SMOOTH_PASS=serial|batched picks the pass kernel (same bits either way) */
bool batchedPassWanted()
{
    const char *e = getenv("MLSGPU_HIP_SMOOTH_PASS");
    return e == nullptr || std::strcmp(e, "serial") != 0;
}

float floatOfBits(Counter bits)
{
    const uint32_t u = (uint32_t) bits;
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_smooth(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                      uint64_t numTriangles, uint32_t iterations, float lambda, float mu, uint32_t boundary,
                                      float *dOutVertices, mlsgpu_smooth_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(lambda) && lambda > 0.0f && lambda <= 1.0f, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(mu) && mu >= -1.0f && mu <= 0.0f, MLSGPU_ERR_INVALID);
    REQUIRE(boundary == MLSGPU_SMOOTH_BOUNDARY_FIXED || boundary == MLSGPU_SMOOTH_BOUNDARY_CURVE, MLSGPU_ERR_INVALID);
    /* the sort's values and tile counts are 32-bit, and so are the indices of a triangle: 6 T < 2^32 */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 5) / 6, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || (dVertices != nullptr && dOutVertices != nullptr), MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->numVertices = numVertices;
    stats->numTriangles = numTriangles;
    stats->passes = (uint64_t) iterations * (mu != 0.0f ? 2 : 1);
    if (numVertices == 0)
    {
        stats->outOfRangeTriangles = numTriangles;      /* every index is >= 0 vertices */
        return MLSGPU_OK;
    }

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t nv = numVertices, nt = numTriangles, n = 6 * nt;
    const SideKeys K = SideKeys::of(nv);
    const dim3 B(256);
    DeviceArray<Counter> counters;
    DeviceArray<float4> workA, workB;
    DeviceArray<uint2> run;
    DeviceArray<uint8_t> onBoundary;
    SortScratch sides;
    DeviceArray<uint32_t> tileSums;
    const uint64_t tileElems = (uint64_t) scanTiles(n) + 1;
    PROPAGATE(counters.alloc(C_WORDS));
    PROPAGATE(workA.alloc(nv));
    PROPAGATE(workB.alloc(nv));
    PROPAGATE(run.alloc(nv));
    PROPAGATE(onBoundary.alloc(nv));
    double scratch = (double) (counters.bytes(C_WORDS) + 2 * workA.bytes(nv) + run.bytes(nv) + onBoundary.bytes(nv));
    if (nt > 0)
    {
        PROPAGATE(sides.alloc(n));
        PROPAGATE(tileSums.alloc(tileElems));
        scratch += (double) (sides.bytes() + tileSums.bytes(tileElems));
    }
    if (ctx->timing)
        ctx->addValue("smooth.scratch.bytes", scratch);

    HIP_CHECK(hipMemsetAsync(counters.get(), 0, C_WORDS * sizeof(Counter), ctx->stream));
    HIP_CHECK(hipMemsetAsync(run.get(), 0, nv * sizeof(uint2), ctx->stream));
    HIP_CHECK(hipMemsetAsync(onBoundary.get(), 0, nv, ctx->stream));
    LAUNCH(ctx, "kernel.smooth.load", loadKernel, dim3(divUp(nv, 256)), B, dVertices, nv, workA.get(), counters.get());
    const uint32_t *neighbours = nullptr;
    if (nt > 0)
    {
        LAUNCH(ctx, "kernel.smooth.records", recordsKernel, dim3(divUp(nt, 256)), B, dTriangles, nt, K, sides.keys(), counters.get());
        Records R;
        PROPAGATE(sides.sort(ctx, "kernel.smooth.sort", K, true, &R));
        /* the neighbour lists, at most one word per record, in the key side that is free again */
        uint32_t *const lists = reinterpret_cast<uint32_t *>(sides.freeKeys());
        neighbours = lists;
        LAUNCH(ctx, "kernel.smooth.mark", markKernel, dim3(std::min(divUp(n, 256), LOOP_BLOCKS)), B, R, onBoundary.get(), counters.get());
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.smooth.adjacency",
                                           KeepIn{R, onBoundary.get(), boundary == MLSGPU_SMOOTH_BOUNDARY_CURVE},
                                           ListOut{R, lists, run.get()}, n, 0u, tileSums.get(), (uint32_t *) nullptr)));
    }
    Counter h[C_WORDS];
    HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h[C_NON_FINITE] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh smooth: %llu vertices have a coordinate that is not finite", h[C_NON_FINITE]);

    /* step 4 */
    const float M = floatOfBits(h[C_INPUT_MAX]);
    const int e = exponentOfBits((uint32_t) h[C_INPUT_MAX]);
    float4 *from = workA.get(), *to = workB.get();
    if (M > 0.0f && nt > 0)
    {
        const double scale = std::ldexp(1.0, 30 - e), invScale = std::ldexp(1.0, e - 30);
        const bool batched = batchedPassWanted();
        for (uint32_t it = 0; it < iterations; it++)
            for (int half = 0; half < (mu != 0.0f ? 2 : 1); half++)
            {
                const double F = (double) (half == 0 ? lambda : mu);
                if (batched)
                    LAUNCH(ctx, "kernel.smooth.pass", passKernel<true>, dim3(divUp(nv, 256)), B, (const float4 *) from, to,
                           (const uint2 *) run.get(), neighbours, nv, scale, invScale, F, counters.get());
                else
                    LAUNCH(ctx, "kernel.smooth.pass", passKernel<false>, dim3(divUp(nv, 256)), B, (const float4 *) from, to,
                           (const uint2 *) run.get(), neighbours, nv, scale, invScale, F, counters.get());
                std::swap(from, to);
            }
    }
    LAUNCH(ctx, "kernel.smooth.finish", finishKernel, dim3(std::min(divUp(nv, 256), LOOP_BLOCKS)), B, dVertices, (const float4 *) from,
           (const uint8_t *) onBoundary.get(), nv, dOutVertices, counters.get());
    HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));

    stats->outOfRangeTriangles = h[C_OUT_OF_RANGE];
    stats->degenerateTriangles = h[C_DEGENERATE];
    stats->numEdges = h[C_EDGES];
    stats->boundaryEdges = h[C_BOUNDARY_EDGES];
    stats->boundaryVertices = h[C_BOUNDARY_VERTICES];
    stats->isolatedVertices = nv - h[C_USED_VERTICES];
    stats->scaleExponent = e;
    const uint64_t moveBits = h[C_MAX_MOVE];
    std::memcpy(&stats->maxMove, &moveBits, sizeof(double));
    stats->maxCoordinate = (double) floatOfBits(std::max(h[C_INPUT_MAX], h[C_PASS_MAX]));
    /* step 7 */
    if (!std::isfinite(stats->maxCoordinate) || stats->maxCoordinate > std::ldexp(1.0, e + 21))
        return setError(MLSGPU_ERR_INVALID, "mesh smooth: diverged, the largest coordinate reached %g (the input's is %g)",
                        stats->maxCoordinate, (double) M);
    return MLSGPU_OK;
}
