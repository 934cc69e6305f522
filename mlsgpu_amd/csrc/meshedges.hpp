/*
 * What the stages that rewrite the edges of a finished mesh in HBM share (flip.hip, collapse.hip), on top of meshpost.hpp: the
 * double vector operations of their contracts, the check for coordinates that are not finite, the triangle quality report,
 * and the sorted side records with every vertex's segment, in which a side's reverse and a vertex's triangles are found.
 */
#ifndef MLSGPU_AMD_MESHEDGES_HPP
#define MLSGPU_AMD_MESHEDGES_HPP

#include "meshpost.hpp"

#include <cmath>

namespace mlsgpu
{

/* The vector operations of their contracts: every one a single correctly rounded double operation, in the order written. */
struct D3
{
    double x, y, z;
};
__device__ __forceinline__ D3 operator-(const D3 &u, const D3 &v) { return D3{u.x - v.x, u.y - v.y, u.z - v.z}; }
__device__ __forceinline__ D3 operator+(const D3 &u, const D3 &v) { return D3{u.x + v.x, u.y + v.y, u.z + v.z}; }
__device__ __forceinline__ double dot(const D3 &u, const D3 &v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ D3 cross(const D3 &u, const D3 &v)
{
    return D3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ __forceinline__ D3 face(const D3 &p, const D3 &q, const D3 &r) { return cross(q - p, r - p); }
__device__ __forceinline__ D3 vertexAt(const float *vertices, uint64_t v)
{
    return D3{(double) vertices[3 * v], (double) vertices[3 * v + 1], (double) vertices[3 * v + 2]};
}

/* a word that other workgroups raise or lower while this one reads it */
__device__ __forceinline__ uint64_t loadWord(const Counter *word)
{
    return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* one quality report's block of counters */
enum
{
    Q_OUT_OF_RANGE = 0,
    Q_DEGENERATE = 1,
    Q_MIN = 2,                  /* ~bits of the smallest q: a maximum, and 0 says that no triangle took part */
    Q_HIST = 3,
    Q_WORDS = Q_HIST + 16
};

namespace
{

/* the coordinates that are not finite, a thread per vertex */
__global__ __launch_bounds__(256) void checkKernel(const float *vertices, uint64_t numVertices, Counter *nonFinite)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= numVertices)
        return;
    tally(!(isfinite(vertices[3 * v]) && isfinite(vertices[3 * v + 1]) && isfinite(vertices[3 * v + 2])), nonFinite);
}

/* Steps 1 and 9 of the flips' contract.  A workgroup loops over the triangles (fewer than 2^32: its counts fit 32 bits), keeps
 * its histogram and its minimum in LDS and sends every word once. */
__global__ __launch_bounds__(256) void qualityKernel(const float *vertices, uint64_t numVertices, const uint32_t *tri,
                                                     uint64_t numTriangles, Counter *report)
{
    __shared__ GroupCounts<2> classes;
    __shared__ uint32_t sHist[16];
    __shared__ Counter sMin;
    if (threadIdx.x < 16)
        sHist[threadIdx.x] = 0;
    if (threadIdx.x == 16)
        sMin = 0;
    classes.clear();
    const int at[2] = {Q_OUT_OF_RANGE, Q_DEGENERATE};
    uint32_t count[2] = {0, 0};
    uint64_t least = 0;         /* ~bits of the smallest q so far */
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < numTriangles; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t t = base + threadIdx.x;
        if (t >= numTriangles)
            continue;
        const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
        const TriangleDefect defect = defectOf(i, numVertices);
        count[0] += defect.outOfRange ? 1u : 0u;
        count[1] += defect.degenerate ? 1u : 0u;
        if (!defect.none())
            continue;
        const D3 p = vertexAt(vertices, i[0]), q = vertexAt(vertices, i[1]), r = vertexAt(vertices, i[2]);
        const D3 x = face(p, q, r), u = q - p, v = r - q, w = p - r;
        const double denominator = (dot(u, u) + dot(v, v)) + dot(w, w);
        double quality = (3.4641016151377544 * sqrt(dot(x, x))) / denominator;
        if (denominator == 0.0 || quality != quality)
            quality = 0.0;
        const double sixteenths = 16.0 * quality;
        atomicAdd(&sHist[sixteenths >= 15.0 ? 15 : (int) sixteenths], 1u);
        least = max(least, ~(uint64_t) __double_as_longlong(quality));
    }
    classes.add(0, count[0]);
    classes.add(1, count[1]);
    const uint64_t ofWave = waveMax64(least);
    if (laneId() == 0 && ofWave != 0)
        atomicMax(&sMin, (Counter) ofWave);
    classes.flush(report, at);          /* (a barrier: sHist and sMin are complete behind it) */
    if (threadIdx.x < 16 && sHist[threadIdx.x] != 0)
        atomicAdd(&report[Q_HIST + threadIdx.x], (Counter) sHist[threadIdx.x]);
    if (threadIdx.x == 16 && sMin != 0)
        atomicMax(&report[Q_MIN], sMin);
}

/* what one quality report's block says, into the fields of a stage's statistics */
inline void qualityOut(const Counter *block, double *minQuality, uint64_t histogram[16])
{
    const uint64_t bits = block[Q_MIN] != 0 ? ~block[Q_MIN] : 0;
    std::memcpy(minQuality, &bits, sizeof(double));
    for (int k = 0; k < 16; k++)
        histogram[k] = block[Q_HIST + k];
}

/* the three directed sides of a triangle; three dead records for one that takes no part */
__global__ __launch_bounds__(256) void recordsKernel(const uint32_t *tri, uint64_t numTriangles, SideKeys K, uint64_t *keys)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    const bool live = defectOf(i, K.numVertices).none();
#pragma unroll
    for (int k = 0; k < 3; k++)
        keys[3 * t + k] = live ? K.keyOf(i[k], i[k == 2 ? 0 : k + 1]) : K.dead();
}

/* run[v] = where the sides that leave v start and end: written by the first and by the last record of v's segment.  Every
 * vertex of a participating triangle has a segment in every round; no other vertex's run is read, unless the stage clears
 * the runs before each classification. */
__global__ __launch_bounds__(256) void segmentsKernel(Records R, uint2 *run)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n)
        return;
    const uint64_t from = R.fromOf(R.keys[i]);
    if (from >= R.numVertices)
        return;
    if (R.segmentStart(i, from))
        run[from].x = (uint32_t) i;
    if (R.segmentEnd(i, from))
        run[from].y = (uint32_t) i + 1;
}

/* the first record of the side from -> to, or R.n: searched in the segment of `from`, a vertex of a participating triangle */
__device__ __forceinline__ uint32_t sideOf(const Records &R, const uint2 *run, uint32_t from, uint32_t to)
{
    const uint2 r = run[from];
    const uint32_t at = R.find(r.x, r.y, R.keyOf(from, to));
    return at != r.y ? at : (uint32_t) R.n;
}

} // namespace

} // namespace mlsgpu

#endif
