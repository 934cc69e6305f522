/*
 * Area-weighted vertex normals of an indexed triangle mesh that is resident in HBM.  The reference has no counterpart: its
 * meshes carry positions and triangles (src/fast_ply.cpp:443-521).  The contract (include/mlsgpu_hip.h, DESIGN.md "Mesh
 * normals") is written so that every output is an integer sum or one correctly rounded operation away from one: the result
 * does not depend on the schedule.
 *
 *   extent      a thread per triangle: the face vector c = (p1 - p0) x (p2 - p0) in doubles, the largest |component| over the
 *               mesh (a 64-bit atomicMax on the bits of the double, one per wave), the triangles that take no part
 *   accumulate  a thread per triangle: c again (same operations, same bits), q = llrint(c * 2^(30 - e)) with e read from the
 *               largest component where the first kernel left it, added to the 64-bit sums of the three corners
 *   finish      a thread per vertex: the sum as doubles, normalised, as floats
 *
 * One stream synchronisation, at the end.  An index >= V is compared and counted, never used as an address.
 *
 * Scratch belongs to the call: 24 bytes per vertex (the sums) and four 64-bit words.
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
    C_NON_FINITE = 1,
    C_ZERO_NORMALS = 2,
    C_MAX_BITS = 3,             /* the bits of the largest |component|, a double */
    C_WORDS = 4
};

const uint32_t NO_VERTEX = 0xFFFFFFFFu;     /* what a lane that adds nothing holds: an index that takes part is < V <= 2^32 - 1 */

struct Face
{
    uint32_t index[3];
    double c[3];
    bool outOfRange, nonFinite;
    __device__ __forceinline__ bool takesPart() const { return !outOfRange && !nonFinite; }
};

/* steps 1 and 2 of the contract; a triangle that takes no part has c = 0 */
__device__ __forceinline__ Face faceOf(const float *vertices, uint64_t numVertices, const uint32_t *triangles, uint64_t t)
{
    Face f;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        f.index[k] = triangles[3 * t + k];
        f.c[k] = 0.0;
    }
    f.outOfRange = f.index[0] >= numVertices || f.index[1] >= numVertices || f.index[2] >= numVertices;
    f.nonFinite = false;
    if (f.outOfRange)
        return f;
    double p[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int axis = 0; axis < 3; axis++)
            p[k][axis] = (double) vertices[3 * (uint64_t) f.index[k] + axis];
    double a[3], b[3];
#pragma unroll
    for (int axis = 0; axis < 3; axis++)
    {
        a[axis] = p[1][axis] - p[0][axis];
        b[axis] = p[2][axis] - p[0][axis];
    }
    const double c[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    f.nonFinite = !(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]));
    if (!f.nonFinite)
#pragma unroll
        for (int k = 0; k < 3; k++)
            f.c[k] = c[k];
    return f;
}

/* Every lane of every wave stays to the end: waveMax64 needs the full wave. */
__global__ __launch_bounds__(256) void extentKernel(const float *vertices, uint64_t numVertices, const uint32_t *triangles,
                                                    uint64_t numTriangles, Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < numTriangles;
    Face f;
    f.outOfRange = f.nonFinite = false;
    f.c[0] = f.c[1] = f.c[2] = 0.0;
    if (live)
        f = faceOf(vertices, numVertices, triangles, t);
    tally(f.outOfRange, &counters[C_OUT_OF_RANGE]);
    tally(f.nonFinite, &counters[C_NON_FINITE]);
    const uint64_t bits = (uint64_t) __double_as_longlong(fmax(fmax(fabs(f.c[0]), fabs(f.c[1])), fabs(f.c[2])));
    const uint64_t most = waveMax64(bits);
    if (laneId() == 0 && most != 0)
        atomicMax(&counters[C_MAX_BITS], (Counter) most);
}

/* step 3 is meshpost.hpp's exponentOfDoubleBits of the largest component; q = llrint(ldexp(component, shift)): ldexp is exact wherever the result is normal, and a result that is not is far below
 * 1/2; rint rounds ties to even */
__device__ __forceinline__ void quantise(const double c[3], int shift, long long q[3])
{
#pragma unroll
    for (int k = 0; k < 3; k++)
        q[k] = (long long) rint(ldexp(c[k], shift));
}

/* nine atomics per triangle that takes part */
__global__ __launch_bounds__(256) void accumulatePlainKernel(const float *vertices, uint64_t numVertices, const uint32_t *triangles,
                                                             uint64_t numTriangles, const Counter *counters, Counter *sums)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t maxBits = counters[C_MAX_BITS];
    if (t >= numTriangles || maxBits == 0)
        return;
    const Face f = faceOf(vertices, numVertices, triangles, t);
    if (!f.takesPart())
        return;
    long long q[3];
    quantise(f.c, 30 - exponentOfDoubleBits(maxBits), q);
#pragma unroll
    for (int corner = 0; corner < 3; corner++)
#pragma unroll
        for (int k = 0; k < 3; k++)
            atomicAdd(&sums[3 * (uint64_t) f.index[corner] + k], (Counter) q[k]);
}

/*
 * The same sums with fewer atomics where neighbouring triangles share a vertex in the same corner (a fan around a hub, the
 * strips of a lattice): per corner, the lanes of a wave form runs of equal vertices; a run adds up by shuffles and its first
 * lane issues the three atomics.  A wave without such a pair in a corner (wave-uniform) goes the plain way for that corner.
 * The sums are integers: the result is the plain kernel's.  No lane leaves early: the shuffles read every lane.
 */
__global__ __launch_bounds__(256) void accumulateWaveKernel(const float *vertices, uint64_t numVertices, const uint32_t *triangles,
                                                            uint64_t numTriangles, const Counter *counters, Counter *sums)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t maxBits = counters[C_MAX_BITS];
    if (maxBits == 0)
        return;                 /* (uniform over the grid) */
    Face f;
    f.outOfRange = true;
    f.nonFinite = false;
    if (t < numTriangles)
        f = faceOf(vertices, numVertices, triangles, t);
    const bool adds = f.takesPart();
    long long q[3] = {0, 0, 0};
    if (adds)
        quantise(f.c, 30 - exponentOfDoubleBits(maxBits), q);
    const uint32_t lane = laneId();
#pragma unroll
    for (int corner = 0; corner < 3; corner++)
    {
        const uint32_t v = adds ? f.index[corner] : NO_VERTEX;
        const uint32_t before = waveShiftUp1(v);
        const bool head = lane == 0 || before != v || !adds;
        if (__ballot(!head) == 0)
        {
            if (adds)
#pragma unroll
                for (int k = 0; k < 3; k++)
                    atomicAdd(&sums[3 * (uint64_t) v + k], (Counter) q[k]);
            continue;
        }
        const uint32_t run = waveInclusiveScan(head ? 1u : 0u);
        long long s[3] = {q[0], q[1], q[2]};
#pragma unroll
        for (int step = 1; step < WAVE; step <<= 1)
        {
            const bool same = __shfl_down(run, step, WAVE) == run && lane + step < WAVE;
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                const long long other = __shfl_down(s[k], step, WAVE);
                s[k] += same ? other : 0;
            }
        }
        if (head && adds)
#pragma unroll
            for (int k = 0; k < 3; k++)
                atomicAdd(&sums[3 * (uint64_t) v + k], (Counter) s[k]);
    }
}

/* step 5 */
__global__ __launch_bounds__(256) void finishKernel(const Counter *sums, uint64_t numVertices, float *normals, Counter *counters)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < numVertices;
    bool zero = false;
    if (live)
    {
        const double x[3] = {(double) (long long) sums[3 * v], (double) (long long) sums[3 * v + 1], (double) (long long) sums[3 * v + 2]};
        const double l2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
        const double l = __dsqrt_rn(l2);
        zero = l == 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++)
            normals[3 * v + k] = zero ? 0.0f : (float) (x[k] / l);
    }
    tally(zero, &counters[C_ZERO_NORMALS]);
}

/* MLSGPU_HIP_NORMALS_ACCUMULATE=plain|wave picks the accumulate kernel (same bits either way) */
bool waveAccumulateWanted()
{
    const char *e = getenv("MLSGPU_HIP_NORMALS_ACCUMULATE");
    return e == nullptr || std::strcmp(e, "plain") != 0;
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_normals(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                       uint64_t numTriangles, float *dOutNormals, mlsgpu_normals_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    /* the indices of a triangle are 32-bit, and so is a launch's grid */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || (dVertices != nullptr && dOutNormals != nullptr), MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->numVertices = numVertices;
    stats->numTriangles = numTriangles;
    if (numVertices == 0 && numTriangles == 0)
        return MLSGPU_OK;

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t nv = numVertices, nt = numTriangles;
    const dim3 B(256);
    DeviceArray<Counter> counters, sums;
    PROPAGATE(counters.alloc(C_WORDS));
    PROPAGATE(sums.alloc(3 * nv));
    if (ctx->timing)
        ctx->addValue("normals.scratch.bytes", (double) (counters.bytes(C_WORDS) + sums.bytes(3 * nv)));
    HIP_CHECK(hipMemsetAsync(counters.get(), 0, C_WORDS * sizeof(Counter), ctx->stream));
    if (nv > 0)
        HIP_CHECK(hipMemsetAsync(sums.get(), 0, 3 * nv * sizeof(Counter), ctx->stream));
    if (nt > 0)
    {
        LAUNCH(ctx, "kernel.normals.extent", extentKernel, dim3(divUp(nt, 256)), B, dVertices, nv, dTriangles, nt, counters.get());
        if (waveAccumulateWanted())
            LAUNCH(ctx, "kernel.normals.accumulate", accumulateWaveKernel, dim3(divUp(nt, 256)), B, dVertices, nv, dTriangles, nt,
                   (const Counter *) counters.get(), sums.get());
        else
            LAUNCH(ctx, "kernel.normals.accumulate", accumulatePlainKernel, dim3(divUp(nt, 256)), B, dVertices, nv, dTriangles, nt,
                   (const Counter *) counters.get(), sums.get());
    }
    if (nv > 0)
        LAUNCH(ctx, "kernel.normals.finish", finishKernel, dim3(divUp(nv, 256)), B, (const Counter *) sums.get(), nv, dOutNormals,
               counters.get());
    Counter hCounters[C_WORDS];
    HIP_CHECK(hipMemcpyAsync(hCounters, counters.get(), sizeof(hCounters), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    stats->outOfRangeTriangles = hCounters[C_OUT_OF_RANGE];
    stats->nonFiniteTriangles = hCounters[C_NON_FINITE];
    stats->zeroNormals = hCounters[C_ZERO_NORMALS];
    stats->scaleExponent = hCounters[C_MAX_BITS] != 0 ? exponentOfDoubleBits(hCounters[C_MAX_BITS]) : 0;
    return MLSGPU_OK;
}
