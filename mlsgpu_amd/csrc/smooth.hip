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
#include "common.hpp"
#include "primitives.hpp"

#include <cmath>
#include <cstdlib>

using namespace mlsgpu;

namespace
{

typedef unsigned long long Counter;

enum
{
    C_OUT_OF_RANGE = 0,
    C_DEGENERATE = 1,
    C_EDGES = 2,
    C_BOUNDARY_EDGES = 3,
    C_USED_VERTICES = 4,        /* vertices with a segment: the others are isolated */
    C_BOUNDARY_VERTICES = 5,
    C_NON_FINITE = 6,           /* input coordinates */
    C_INPUT_MAX = 7,            /* the bits of the largest |coordinate| of the input: non-negative floats order as their bits, */
    C_PASS_MAX = 8,             /* ... of the passes' outputs                                        and a NaN above infinity */
    C_MAX_MOVE = 9,             /* the bits of the largest move, a double */
    C_WORDS = 10
};

const double CLAMP = 4611686018427387904.0;     /* 2^62: what a value is clamped to before it becomes an integer */

/* The lanes of the wave for which `hit` holds add their number to *count with one atomic. */
__device__ __forceinline__ void tally(bool hit, Counter *count)
{
    const uint64_t mask = __ballot(hit);
    if (hit && popcBelow(mask) == 0)
        atomicAdd(count, (Counter) __popcll(mask));
}

__device__ __forceinline__ uint32_t absBits(float x) { return __float_as_uint(fabsf(x)); }

/* What a launch may use of the device for a kernel whose workgroups loop over the elements: a count or a maximum that every
 * wave of a thread-per-element grid sends to ONE address costs about 10 ns apiece there (the atomics of one address are
 * served one after the other), 10 ms for the 22 M records of a 4 M-triangle chunk; these workgroups add up in registers and
 * LDS and send one atomic each. */
const uint32_t LOOP_BLOCKS = 1024;

/* the largest of the wave's bit patterns into *word; needs the full wave.  The word is read first: a maximum is reached by
 * the first few waves, and the others then have nothing to send (a stale read costs an atomic, never the result). */
__device__ __forceinline__ void foldMax(uint32_t bits, Counter *word)
{
    const uint32_t most = waveMax(bits);
    if (laneId() == 0 && (Counter) most > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(word, (Counter) most);
}

/* Every lane of every wave stays to the end: waveMax needs the full wave. */
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

/* steps 1 and 2 of the contract.  The six records of a triangle that takes no part get from = V: they sort behind every
 * other record and nothing follows them. */
__global__ __launch_bounds__(256) void recordsKernel(const uint32_t *tri, uint64_t numTriangles, uint64_t numVertices, uint32_t b,
                                                     uint64_t *keys, Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    const bool outOfRange = i[0] >= numVertices || i[1] >= numVertices || i[2] >= numVertices;
    const bool degenerate = !outOfRange && (i[0] == i[1] || i[1] == i[2] || i[2] == i[0]);
    tally(outOfRange, &counters[C_OUT_OF_RANGE]);
    tally(degenerate, &counters[C_DEGENERATE]);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const uint64_t from = i[k], to = i[k == 2 ? 0 : k + 1];
        const bool part = !outOfRange && !degenerate;
        keys[6 * t + 2 * k] = part ? (from << b) | to : numVertices << b;
        keys[6 * t + 2 * k + 1] = part ? (to << b) | from : numVertices << b;
    }
}

/* the sorted records */
struct Records
{
    const uint64_t *keys;
    uint64_t n;
    uint64_t numVertices;
    uint32_t b;

    __device__ __forceinline__ uint64_t fromOf(uint64_t key) const { return key >> b; }
    __device__ __forceinline__ uint32_t toOf(uint64_t key) const { return (uint32_t) (key & ((uint64_t(1) << b) - 1)); }
    __device__ __forceinline__ bool head(uint64_t i, uint64_t key) const { return i == 0 || keys[i - 1] != key; }
    /* the only record of its run: exactly one triangle side uses the edge */
    __device__ __forceinline__ bool single(uint64_t i, uint64_t key) const
    {
        return head(i, key) && (i + 1 == n || keys[i + 1] != key);
    }
};

/* step 2.  Both directions of every side are there, so each end of a boundary edge is marked by the record that leaves it; an
 * edge is counted by the direction that rises.  The plain byte stores race only with stores of the same value.  A workgroup
 * loops over the records (at most 2^32 / LOOP_BLOCKS of them: its counts fit 32 bits) and sends its three counts once. */
__global__ __launch_bounds__(256) void markKernel(Records R, uint8_t *onBoundary, Counter *counters)
{
    __shared__ uint32_t sums[3];
    if (threadIdx.x < 3)
        sums[threadIdx.x] = 0;
    __syncthreads();
    uint32_t count[3] = {0, 0, 0};      /* edges, boundary edges, vertices with a segment: C_EDGES onwards */
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
        count[2] += i == 0 || R.fromOf(R.keys[i - 1]) != from ? 1u : 0u;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const uint32_t ofWave = waveSum(count[k]);
        if (laneId() == 0 && ofWave != 0)
            atomicAdd(&sums[k], ofWave);
    }
    __syncthreads();
    if (threadIdx.x < 3 && sums[threadIdx.x] != 0)
        atomicAdd(&counters[C_EDGES + threadIdx.x], (Counter) sums[threadIdx.x]);
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
        if (i == 0 || R.fromOf(R.keys[i - 1]) != from)
            run[from].x = before;
        if (i + 1 == R.n || R.fromOf(R.keys[i + 1]) != from)
            run[from].y = before + kept;
    }
};

/* Q of step 5: the multiplication by a power of two is ldexp (exact: a float times 2^(30 - e) is a normal double or zero);
 * rint rounds ties to even.  The clamp changes no value of a call that has not diverged (those are below 2^52) and makes the
 * conversion of every other one defined: fmax / fmin hand back the bound for a NaN. */
__device__ __forceinline__ unsigned long long quantise(float x, double scale)
{
    return (unsigned long long) (long long) rint(fmin(fmax((double) x * scale, -CLAMP), CLAMP));
}

/* Step 5.  One aligned 16-byte load per neighbour; the sums are unsigned, so that they wrap.  Every lane stays to the end.
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
                        S[0] += has[i] ? quantise(q[i].x, scale) : 0ull;
                        S[1] += has[i] ? quantise(q[i].y, scale) : 0ull;
                        S[2] += has[i] ? quantise(q[i].z, scale) : 0ull;
                    }
                }
            else
                for (uint32_t j = r.x; j < r.y; j++)
                {
                    const float4 q = in[neighbours[j]];
                    S[0] += quantise(q.x, scale);
                    S[1] += quantise(q.y, scale);
                    S[2] += quantise(q.z, scale);
                }
            const float own[3] = {p.x, p.y, p.z};
            float moved[3];
#pragma unroll
            for (int a = 0; a < 3; a++)
            {
                const long long D = (long long) (S[a] - (unsigned long long) k * quantise(own[a], scale));
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
    __shared__ uint32_t sBoundary;
    __shared__ Counter sMove;
    if (threadIdx.x == 0)
    {
        sBoundary = 0;
        sMove = 0;
    }
    __syncthreads();
    uint32_t boundary = 0;
    uint64_t bits = 0;          /* of the largest move: non-negative doubles order as their bits, and a NaN above infinity */
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
    const uint32_t ofWave = waveSum(boundary);
    /* the largest 64-bit pattern of the wave: the largest high word, then the largest low word among its holders */
    const uint32_t hi = waveMax((uint32_t) (bits >> 32));
    const uint32_t lo = waveMax((uint32_t) (bits >> 32) == hi ? (uint32_t) bits : 0u);
    if (laneId() == 0)
    {
        if (ofWave != 0)
            atomicAdd(&sBoundary, ofWave);
        atomicMax(&sMove, (Counter) ((uint64_t) hi << 32 | lo));
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        if (sBoundary != 0)
            atomicAdd(&counters[C_BOUNDARY_VERTICES], (Counter) sBoundary);
        if (sMove != 0)
            atomicMax(&counters[C_MAX_MOVE], sMove);
    }
}

uint32_t bitLength(uint64_t v)
{
    uint32_t b = 0;
    while (v != 0)
    {
        b++;
        v >>= 1;
    }
    return b;
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
    const uint32_t b = bitLength(nv);           /* V itself fits: the key of the records that take no part */
    const dim3 B(256);
    DeviceArray<Counter> counters;
    DeviceArray<float4> workA, workB;
    DeviceArray<uint2> run;
    DeviceArray<uint8_t> onBoundary;
    DeviceArray<uint64_t> keysA, keysB;
    DeviceArray<uint32_t> valsA, valsB, hist, tileSums;
    const uint64_t histElems = sortHistElems(n), tileElems = (uint64_t) scanTiles(n) + 1;
    PROPAGATE(counters.alloc(C_WORDS));
    PROPAGATE(workA.alloc(nv));
    PROPAGATE(workB.alloc(nv));
    PROPAGATE(run.alloc(nv));
    PROPAGATE(onBoundary.alloc(nv));
    double scratch = (double) (counters.bytes(C_WORDS) + 2 * workA.bytes(nv) + run.bytes(nv) + onBoundary.bytes(nv));
    if (nt > 0)
    {
        PROPAGATE(keysA.alloc(n));
        PROPAGATE(keysB.alloc(n));
        PROPAGATE(valsA.alloc(n));
        PROPAGATE(valsB.alloc(n));
        PROPAGATE(hist.alloc(histElems));
        PROPAGATE(tileSums.alloc(tileElems));
        scratch += (double) (2 * keysA.bytes(n) + 2 * valsA.bytes(n) + hist.bytes(histElems) + tileSums.bytes(tileElems));
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
        LAUNCH(ctx, "kernel.smooth.records", recordsKernel, dim3(divUp(nt, 256)), B, dTriangles, nt, nv, b, keysA.get(), counters.get());
        SortResult<uint64_t> sorted = {nullptr, nullptr};
        PROPAGATE(radixSort<uint64_t>(ctx, "kernel.smooth.sort", keysA, valsA, keysB, valsB, n, 2 * b, true, hist, nullptr, &sorted));
        /* the key side that does not hold the result is free again: the neighbour lists, at most one word per record */
        uint32_t *const lists = reinterpret_cast<uint32_t *>(sorted.keys == keysA.get() ? keysB.get() : keysA.get());
        neighbours = lists;
        const Records R = {sorted.keys, n, nv, b};
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
    int e = 0;
    if (M > 0.0f)
        e = std::ilogb(M);              /* 2^e <= M < 2^(e + 1), a subnormal's true exponent */
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
