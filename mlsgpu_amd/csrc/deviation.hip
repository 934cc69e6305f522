/*
 * The deviation report of a set of points against an indexed triangle mesh, both resident in HBM: for every point the squared
 * distance to the mesh's surface, exact up to a search distance D, and the statistics of those distances.  The reference has no
 * counterpart.  The contract (include/mlsgpu_hip.h, DESIGN.md "Mesh deviation") fixes every floating-point operation and makes
 * every field of the report a count, a minimum, a maximum or an integer sum: the result depends neither on the schedule nor on
 * anything below that the contract does not name -- the grid's cell size least of all.
 *
 *   grid       the target's triangles that take part (step 1), each in the cells its box, inflated by D, touches, as
 *              (cell key, triangle) pairs sorted by cell key: meshgrid.hpp, with reach = D
 *   sort       the points, with their own cell's key, by that key too
 *   distance   over the sorted points: the point's cell's run of pairs by binary search, step 2 and step 3 for each of them,
 *              (best, triangle) as a lexicographic minimum in registers -- one lane per point, or a power of two of
 *              neighbouring lanes that share the run and combine by shuffles: step 4 needs no atomics
 *   report     over the points' results: the counts, the histogram, the fixed-point sum and the maximum; then the lowest
 *              point that attains the maximum                                                            -- one read-back --
 *
 * Why a point needs only its own cell.  cell() is monotone (meshgrid.hpp), and a triangle goes into every cell from
 * cell(lo - D) to cell(hi + D) per axis, with the SAME rounded doubles lo - D and hi + D that step 2 compares with.  For a
 * candidate pair lo - D <= p <= hi + D, so cell(lo - D) <= cell(p) <= cell(hi + D) on every axis: the pair is among those of
 * the point's cell, whatever h and the origin are.  The kernel applies step 2 to every pair it is handed, so a superset is all
 * it needs.
 *
 * Scratch belongs to the call: 24 bytes per point (the two sides of the sort's 64-bit keys and 32-bit values), 8 more where the
 * caller does not take the distances, 8 bytes per triangle (its cell count and where its pairs begin), 24 bytes per grid pair,
 * the sorts' histograms (4 KB per 4096 records) and the scan's tile sums.  The pairs are at most max(2^20, 8 T).
 */
#include "meshgrid.hpp"

#include <cmath>
#include <cstdlib>

using namespace mlsgpu;

namespace
{

enum
{
    C_BAD_POINTS = G_WORDS,     /* point coordinates that are not finite */
    C_WITHIN,
    C_BEYOND,
    C_HISTOGRAM,                /* 16 */
    C_SUM_Q = C_HISTOGRAM + 16,
    C_MAX_D2,                   /* the bits of the largest distance */
    C_FARTHEST,
    C_HANDED,                   /* a timed call: the pairs the distance kernel was handed, and ... */
    C_CANDIDATES,               /* ... those of them that passed step 2 */
    C_FARTHEST_TIES,            /* the points that attain the maximum (tally() counts what it finds the first of) */
    C_WORDS
};

const GridNames NAMES = {"mesh deviation", "pairs", "kernel.deviation.extent", "kernel.deviation.classify", "kernel.deviation.count",
                         "kernel.deviation.scan", "kernel.deviation.emit", "kernel.deviation.sort", "deviation.pairs", "deviation.cellsize"};

const uint32_t NO_TRIANGLE = 0xFFFFFFFFu;
const uint64_t SPREAD_THREADS = uint64_t(1) << 20;      /* a point's run is dealt out to several lanes below this many lanes in all */

struct Corners
{
    float a[3], b[3], c[3];
};

/* the corners of triangle t of a target whose indices are known to be in range */
__device__ __forceinline__ Corners cornersOf(const float *vertices, const uint32_t *tri, uint64_t t)
{
    const uint64_t i = tri[3 * t], j = tri[3 * t + 1], k = tri[3 * t + 2];
    Corners T;
#pragma unroll
    for (int x = 0; x < 3; x++)
    {
        T.a[x] = vertices[3 * i + x];
        T.b[x] = vertices[3 * j + x];
        T.c[x] = vertices[3 * k + x];
    }
    return T;
}

/* step 2's bounds of one axis: lo - D and hi + D, one double operation each */
__device__ __forceinline__ void reachOf(const Corners &T, int axis, double D, double *from, double *to)
{
    const float lo = fminf(fminf(T.a[axis], T.b[axis]), T.c[axis]);
    const float hi = fmaxf(fmaxf(T.a[axis], T.b[axis]), T.c[axis]);
    *from = (double) lo - D;
    *to = (double) hi + D;
}

/* ---------------------------------------------------------------- step 3 */

struct D3
{
    double x, y, z;
};
__device__ __forceinline__ D3 sub(const D3 &u, const D3 &v) { return D3{u.x - v.x, u.y - v.y, u.z - v.z}; }
__device__ __forceinline__ double dot(const D3 &u, const D3 &v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
__device__ __forceinline__ D3 cross(const D3 &u, const D3 &v)
{
    return D3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}
__device__ __forceinline__ D3 widen(const float f[3]) { return D3{(double) f[0], (double) f[1], (double) f[2]}; }

__device__ __forceinline__ double seg(const D3 &p, const D3 &a, const D3 &b)
{
    const D3 u = sub(b, a), w = sub(p, a);
    const double L = dot(u, u);
    double s = (L == 0.0) ? 0.0 : dot(w, u) / L;
    s = fmin(fmax(s, 0.0), 1.0);
    const D3 r = D3{w.x - s * u.x, w.y - s * u.y, w.z - s * u.z};
    return dot(r, r);
}

__device__ __forceinline__ double face(const D3 &p, const D3 &a, const D3 &b, const D3 &c)
{
    const D3 ab = sub(b, a), pa = sub(p, a);
    const D3 n = cross(ab, sub(c, a));
    const double nn = dot(n, n);
    const double i0 = dot(cross(ab, pa), n);
    const double i1 = dot(cross(sub(c, b), sub(p, b)), n);
    const double i2 = dot(cross(sub(a, c), sub(p, c)), n);
    if (nn > 0.0 && i0 >= 0.0 && i1 >= 0.0 && i2 >= 0.0)
    {
        const double h = dot(pa, n);
        return (h * h) / nn;
    }
    return __builtin_huge_val();
}

__device__ __forceinline__ double distance2(const D3 &p, const Corners &T)
{
    const D3 a = widen(T.a), b = widen(T.b), c = widen(T.c);
    return fmin(fmin(fmin(seg(p, a, b), seg(p, b, c)), seg(p, c, a)), face(p, a, b, c));
}

/* ---------------------------------------------------------------- kernels */

__global__ __launch_bounds__(256) void pointKeysKernel(Grid G, const float *points, uint64_t numPoints, uint64_t *keys)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numPoints)
        return;
    keys[i] = G.key(G.cell(0, (double) points[3 * i]), G.cell(1, (double) points[3 * i + 1]), G.cell(2, (double) points[3 * i + 2]));
}

/* the first pair of the cell's run and the one behind its last: two binary searches, at most 32 halvings each */
__device__ __forceinline__ void runOf(const uint64_t *keys, uint32_t n, uint64_t key, uint32_t *from, uint32_t *to)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    *from = lo;
    hi = n;
    while (lo < hi)
    {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] <= key) lo = mid + 1; else hi = mid;
    }
    *to = lo;
}

/* Steps 2 to 4.  The points come in the order of their cells, so that the lanes of a wave walk the same run of pairs and load
 * the same triangles.  2^laneShift neighbouring lanes share one point and deal its run out among themselves, pair k to lane
 * k mod 2^laneShift: few points with long runs still fill the device.  Each keeps (best, triangle) as a lexicographic minimum
 * from (+infinity, 0xFFFFFFFF) on, and the minimum over the sharers -- a butterfly of shuffles; a minimum does not care how it
 * is bracketed -- is step 4's: the smallest distance, then the lowest index that attains it.  (A candidate at +infinity wins
 * against the start by its index, as step 4 has it; the point is beyond either way.)  The pairs' triangles all take part
 * (emit wrote them), so their indices are addresses.  Every lane stays to the end, for the shuffles and for `pairTally` (a
 * timed call): the wave adds up how many pairs it was handed and how many were candidates, and sends each sum once. */
__global__ __launch_bounds__(256) void distanceKernel(const float *points, const uint64_t *pointKeys, const uint32_t *pointOrder,
                                                      uint64_t numPoints, uint32_t laneShift, const float *vertices, const uint32_t *tri,
                                                      const uint64_t *pairKeys, const uint32_t *pairTriangles, uint32_t numPairs, double D,
                                                      double *distance2Out, uint32_t *nearestOut, Counter *pairTally)
{
    const uint64_t thread = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t i = thread >> laneShift;
    const uint32_t sharers = 1u << laneShift, sub = (uint32_t) thread & (sharers - 1);
    long long handed = 0, candidates = 0;
    double best = __builtin_huge_val();
    uint32_t nearest = NO_TRIANGLE, point = 0;
    if (i < numPoints)
    {
        point = pointOrder[i];
        const float pf[3] = {points[3 * (uint64_t) point], points[3 * (uint64_t) point + 1], points[3 * (uint64_t) point + 2]};
        const D3 p = widen(pf);
        uint32_t from, to;
        runOf(pairKeys, numPairs, pointKeys[i], &from, &to);
        for (uint64_t k = (uint64_t) from + sub; k < to; k += sharers)
        {
            handed++;
            const uint32_t t = pairTriangles[k];
            const Corners T = cornersOf(vertices, tri, t);
            bool candidate = true;
#pragma unroll
            for (int x = 0; x < 3; x++)
            {
                double lo, hi;
                reachOf(T, x, D, &lo, &hi);
                const double px = x == 0 ? p.x : x == 1 ? p.y : p.z;
                candidate = candidate && lo <= px && px <= hi;
            }
            if (!candidate)
                continue;
            candidates++;
            const double d = distance2(p, T);
            if (d < best || (d == best && t < nearest))
            {
                best = d;
                nearest = t;
            }
        }
    }
    for (uint32_t step = 1; step < sharers; step <<= 1)
    {
        const double d = __shfl_xor(best, (int) step, WAVE);
        const uint32_t t = (uint32_t) __shfl_xor((int) nearest, (int) step, WAVE);
        if (d < best || (d == best && t < nearest))
        {
            best = d;
            nearest = t;
        }
    }
    if (i < numPoints && sub == 0)
    {
        const bool within = nearest != NO_TRIANGLE && best <= D * D;
        distance2Out[point] = within ? best : __builtin_huge_val();
        if (nearestOut != nullptr)
            nearestOut[point] = within ? nearest : NO_TRIANGLE;
    }
    if (pairTally != nullptr)
    {
        const long long handedOfWave = waveSum64(handed), candidatesOfWave = waveSum64(candidates);
        if (laneId() == 0)
        {
            atomicAdd(&pairTally[0], (Counter) handedOfWave);
            atomicAdd(&pairTally[1], (Counter) candidatesOfWave);
        }
    }
}

/* every point beyond: a target without a triangle that takes part */
__global__ __launch_bounds__(256) void beyondKernel(uint64_t numPoints, double *distance2Out, uint32_t *nearestOut)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numPoints)
        return;
    distance2Out[i] = __builtin_huge_val();
    if (nearestOut != nullptr)
        nearestOut[i] = NO_TRIANGLE;
}

/* Step 5 but for the farthest point.  A workgroup loops over blocks of 256 points -- every lane as often, the wave whole --
 * and sends once.  Lane k < 16 of a wave keeps bin k's count.  What one workgroup counts fits 32 bits (P < 2^32). */
__global__ __launch_bounds__(256) void reportKernel(const double *distance2In, uint64_t numPoints, double D2, double scale, Counter *counters)
{
    enum { WITHIN, BEYOND, BIN, SUMS = BIN + 16 };
    __shared__ GroupCounts<SUMS> totals;
    totals.clear();
    int at[SUMS];
    at[WITHIN] = C_WITHIN;
    at[BEYOND] = C_BEYOND;
#pragma unroll
    for (int k = 0; k < 16; k++)
        at[BIN + k] = C_HISTOGRAM + k;
    const uint32_t lane = laneId();
    uint32_t within = 0, beyond = 0, ofBin = 0;
    long long sumQ = 0;
    uint64_t most = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < numPoints; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i = base + threadIdx.x;
        const double best = i < numPoints ? distance2In[i] : __builtin_huge_val();
        const bool in = i < numPoints && best <= D2;    /* a point beyond holds +infinity */
        within += in ? 1u : 0u;
        beyond += i < numPoints && !in ? 1u : 0u;
        uint32_t bin = 0;
        if (in)
        {
#pragma unroll
            for (uint32_t k = 1; k < 16; k++)
                bin = best >= (D2 * (double) (k * k)) / 256.0 ? k : bin;
            sumQ += (long long) rint(best * scale);
            most = max(most, (uint64_t) __double_as_longlong(best));
        }
#pragma unroll
        for (uint32_t k = 0; k < 16; k++)
        {
            const uint32_t n = (uint32_t) __popcll(__ballot(in && bin == k));
            ofBin += lane == k ? n : 0u;
        }
    }
    totals.add(WITHIN, within);
    totals.add(BEYOND, beyond);
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
        totals.add(BIN + (int) k, lane == k ? ofBin : 0u);
    const long long sumOfWave = waveSum64(sumQ);
    const uint64_t mostOfWave = waveMax64(most);
    if (lane == 0)
    {
        if (sumOfWave != 0)
            atomicAdd(&counters[C_SUM_Q], (Counter) sumOfWave);
        if (mostOfWave != 0)
            atomicMax(&counters[C_MAX_D2], (Counter) mostOfWave);
    }
    totals.flush(counters, at);
}

/* the lowest point that attains the maximum: few do, so one atomic per wave that has one */
__global__ __launch_bounds__(256) void farthestKernel(const double *distance2In, uint64_t numPoints, Counter *counters)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool hit = i < numPoints && counters[C_WITHIN] != 0 && (Counter) __double_as_longlong(distance2In[i]) == counters[C_MAX_D2];
    tally(hit, &counters[C_FARTHEST_TIES], i, &counters[C_FARTHEST]);
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_deviation(mlsgpu_ctx *ctx, const float *dPoints, uint64_t numPoints, const float *dVertices,
                                         uint64_t numVertices, const uint32_t *dTriangles, uint64_t numTriangles, float maxDistance,
                                         double *dDistance2, uint32_t *dNearest, mlsgpu_deviation *out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(maxDistance) && maxDistance > 0.0f, MLSGPU_ERR_INVALID);
    /* the sorts' values and the indices of a triangle are 32-bit */
    REQUIRE(numPoints < (uint64_t(1) << 32) && numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3,
            MLSGPU_ERR_LENGTH);
    REQUIRE(numPoints == 0 || dPoints != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(numVertices == 0 || dVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    const uint64_t np = numPoints, nv = numVertices, nt = numTriangles;
    const double D = (double) maxDistance, D2 = D * D;
    uint64_t bitsOfD2;
    std::memcpy(&bitsOfD2, &D2, sizeof(D2));
    const int e = exponentOfDoubleBits(bitsOfD2);
    std::memset(out, 0, sizeof(*out));
    out->numPoints = np;
    out->numVertices = nv;
    out->numTriangles = nt;
    out->farthestPoint = UINT64_MAX;
    out->scaleExponent = np > 0 ? e : 0;
    out->limit2 = D2;

    HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 B(256);
    CounterBlock counters;
    PROPAGATE(counters.start(ctx, C_WORDS, {C_FARTHEST}));
    const std::vector<Counter> &h = counters.h;         /* what the last read-back found */
    TriangleGrid grid = {ctx, NAMES, counters, dVertices, nv, dTriangles, nt, D};
    PROPAGATE(grid.measure(dPoints, np, C_BAD_POINTS));
    if (grid.badPoints != 0 || grid.badVertices != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh deviation: %llu point and %llu target coordinates are not finite",
                        (unsigned long long) grid.badPoints, (unsigned long long) grid.badVertices);
    out->outOfRangeTriangles = grid.outOfRange;
    out->degenerateTriangles = grid.degenerate;
    if (np == 0)
        return MLSGPU_OK;

    DeviceArray<double> ownDistance2;
    if (dDistance2 == nullptr)
    {
        PROPAGATE(ownDistance2.alloc(np));
        dDistance2 = ownDistance2.get();
    }
    double scratch = (double) (counters.bytes() + (ownDistance2.get() != nullptr ? ownDistance2.bytes(np) : 0));
    SortScratch sortedPoints;
    if (grid.live == 0)
        LAUNCH(ctx, "kernel.deviation.distance", beyondKernel, dim3(divUp(np, 256)), B, np, dDistance2, dNearest);
    else
    {
        PROPAGATE(sortedPoints.alloc(np));
        PROPAGATE(grid.build(grid.firstCell(), nullptr));
        scratch += (double) (grid.bytes() + sortedPoints.bytes());
        /* (both sorts under one name: a launch site of the sort keeps one stat id per translation unit) */
        SortResult<uint64_t> pointsByCell = {nullptr, nullptr};
        LAUNCH(ctx, "kernel.deviation.pointkeys", pointKeysKernel, dim3(divUp(np, 256)), B, grid.G, dPoints, np, sortedPoints.keys());
        PROPAGATE(radixSort<uint64_t>(ctx, "kernel.deviation.sort", sortedPoints.keysA, sortedPoints.valsA, sortedPoints.keysB,
                                      sortedPoints.valsB, np, grid.G.keyBits(), true, sortedPoints.hist, nullptr, &pointsByCell));
        /* lanes per point: a power of two, as many as keep the launch under SPREAD_THREADS lanes.  (MLSGPU_HIP_DEVIATION_LANES
         * is a tuning aid; the result does not depend on it.) */
        uint32_t laneShift = 0;
        while (laneShift < 6 && (np << (laneShift + 1)) <= SPREAD_THREADS)
            laneShift++;
        if (const char *forced = getenv("MLSGPU_HIP_DEVIATION_LANES"))
        {
            const int lanes = atoi(forced);
            if (lanes >= 1 && lanes <= WAVE && (lanes & (lanes - 1)) == 0)
                laneShift = bitLength((uint64_t) lanes) - 1;
        }
        if (ctx->timing)
            ctx->addValue("deviation.lanes", (double) (1u << laneShift));
        LAUNCH(ctx, "kernel.deviation.distance", distanceKernel, dim3(divUp(np << laneShift, 256)), B, dPoints,
               (const uint64_t *) pointsByCell.keys, (const uint32_t *) pointsByCell.vals, np, laneShift, dVertices, dTriangles,
               (const uint64_t *) grid.byCell.keys, (const uint32_t *) grid.byCell.vals, (uint32_t) grid.numRecords, D, dDistance2, dNearest,
               ctx->timing ? &counters.get()[C_HANDED] : (Counter *) nullptr);
    }
    if (ctx->timing)
        ctx->addValue("deviation.scratch.bytes", scratch);


    LAUNCH(ctx, "kernel.deviation.report", reportKernel, dim3(std::min(divUp(np, 256), LOOP_BLOCKS)), B, (const double *) dDistance2, np, D2,
           powerOfTwo(30 - e), counters.get());
    LAUNCH(ctx, "kernel.deviation.report", farthestKernel, dim3(divUp(np, 256)), B, (const double *) dDistance2, np, counters.get());
    PROPAGATE(counters.readBack(ctx));          /* the scratch goes with the call */
    if (ctx->timing)
    {
        ctx->addValue("deviation.pairs.handed", (double) h[C_HANDED]);
        ctx->addValue("deviation.pairs.candidates", (double) h[C_CANDIDATES]);
    }
    out->within = h[C_WITHIN];
    out->beyond = h[C_BEYOND];
    for (int k = 0; k < 16; k++)
        out->histogram[k] = h[C_HISTOGRAM + k];
    out->sumQ = (int64_t) h[C_SUM_Q];
    std::memcpy(&out->maxDistance2, &h[C_MAX_D2], sizeof(double));
    if (out->within > 0)
        out->farthestPoint = h[C_FARTHEST];
    return MLSGPU_OK;
}
