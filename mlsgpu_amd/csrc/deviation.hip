/*
 * The deviation report of a set of points against an indexed triangle mesh, both resident in HBM: for every point the squared
 * distance to the mesh's surface, exact up to a search distance D, and the statistics of those distances.  The reference has no
 * counterpart.  The contract (include/mlsgpu_hip.h, DESIGN.md "Mesh deviation") fixes every floating-point operation and makes
 * every field of the report a count, a minimum, a maximum or an integer sum: the result depends neither on the schedule nor on
 * anything below that the contract does not name -- the grid's cell size least of all.
 *
 *   extent     over the coordinates of the points and of the target: those that are not finite, and the target's bounding box
 *                                                                                                        -- one read-back --
 *   classify   over the triangles: which take no part (step 1), and the fixed-point sum of the bounding-box extents of the
 *              others, whose mean sizes the first cell                                                   -- one read-back --
 *   count      a thread per triangle: the cells its box, inflated by D, touches.  The host doubles the cell size and counts
 *              again until the pairs fit their budget                                          -- one read-back per size --
 *   emit       a scan over the counts, then a thread per triangle writes its (cell key, triangle) pairs
 *   sort       the pairs by cell key; the points, with their own cell's key, by that key too
 *   distance   over the sorted points: the point's cell's run of pairs by binary search, step 2 and step 3 for each of them,
 *              (best, triangle) as a lexicographic minimum in registers -- one lane per point, or a power of two of
 *              neighbouring lanes that share the run and combine by shuffles: step 4 needs no atomics
 *   report     over the points' results: the counts, the histogram, the fixed-point sum and the maximum; then the lowest
 *              point that attains the maximum                                                            -- one read-back --
 *
 * Why a point needs only its own cell.  cell(x) = clamp(floor((x - origin) / h), 0, n - 1) is three correctly rounded, monotone
 * steps, hence monotone in x.  A triangle goes into every cell from cell(lo - D) to cell(hi + D) per axis, with the SAME rounded
 * doubles lo - D and hi + D that step 2 compares with.  For a candidate pair lo - D <= p <= hi + D, so cell(lo - D) <= cell(p)
 * <= cell(hi + D) on every axis: the pair is among those of the point's cell, whatever h and the origin are.  The kernel applies
 * step 2 to every pair it is handed, so a superset is all it needs.
 *
 * An index >= V is compared and counted, never used as an address; no address depends on a coordinate except through cell(),
 * which is clamped to the grid.
 *
 * Scratch belongs to the call: 24 bytes per point (the two sides of the sort's 64-bit keys and 32-bit values), 8 more where the
 * caller does not take the distances, 8 bytes per triangle (its cell count and where its pairs begin), 24 bytes per grid pair,
 * the sorts' histograms (4 KB per 4096 records) and the scan's tile sums.  The pairs are at most max(2^20, 8 T).
 */
#include "meshpost.hpp"

#include <cmath>
#include <cstdlib>

using namespace mlsgpu;

namespace
{

enum
{
    C_BAD_POINTS = 0,           /* point coordinates that are not finite */
    C_BAD_VERTICES = 1,         /* target coordinates that are not finite */
    C_OUT_OF_RANGE = 2,
    C_DEGENERATE = 3,
    C_LIVE = 4,                 /* triangles that take part */
    C_EXTENT = 5,               /* the fixed-point sum of their extents */
    C_PAIRS = 6,                /* the pairs of the last count */
    C_BOX_MIN = 7,              /* 3: the smallest target coordinate per axis, as ordered bits */
    C_BOX_MAX = 10,             /* 3: the largest */
    C_WITHIN = 13,
    C_BEYOND = 14,
    C_HISTOGRAM = 15,           /* 16 */
    C_SUM_Q = 31,
    C_MAX_D2 = 32,              /* the bits of the largest distance */
    C_FARTHEST = 33,
    C_HANDED = 34,              /* a timed call: the pairs the distance kernel was handed, and ... */
    C_CANDIDATES = 35,          /* ... those of them that passed step 2 */
    C_FARTHEST_TIES = 36,       /* the points that attain the maximum (tally() counts what it finds the first of) */
    C_WORDS = 37
};

const uint32_t NO_TRIANGLE = 0xFFFFFFFFu;
const uint64_t MIN_PAIR_BUDGET = uint64_t(1) << 20;
const uint32_t PAIRS_PER_TRIANGLE = 8;          /* the budget: what the pairs may cost per triangle of the target */
const uint32_t CELL_CAP = 1u << 21;             /* cells per axis: simplify's 21 bits */
const uint64_t SPREAD_THREADS = uint64_t(1) << 20;      /* a point's run is dealt out to several lanes below this many lanes in all */
const int WAVE_LANES = 64;
const uint32_t EXTENT_BITS = 20;                /* a triangle's extent as a fraction of the box's, in the classify sum */

/* floats to integers of the same order (and back): what atomicMin / atomicMax take */
__host__ __device__ inline uint32_t orderedBits(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
inline float fromOrdered(uint32_t o)
{
    const uint32_t bits = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    return f;
}

/* The sparse grid: cell (x, y, z) has the key z << (bx + by) | y << bx | x, the axes as wide as their cell counts need. */
struct Grid
{
    double origin[3];           /* the target's box, lowered by D */
    double h;
    uint32_t n[3];              /* cells per axis, each >= 1 and <= CELL_CAP */
    uint32_t shiftY, shiftZ;
    double D;

    /* monotone in x: one subtraction, one division, floor, clamp */
    __device__ __forceinline__ uint32_t cell(int axis, double x) const
    {
        const double c = floor((x - origin[axis]) / h);
        return (uint32_t) fmin(fmax(c, 0.0), (double) (n[axis] - 1));
    }
    __device__ __forceinline__ uint64_t key(uint32_t x, uint32_t y, uint32_t z) const
    {
        return (uint64_t) z << shiftZ | (uint64_t) y << shiftY | x;
    }
};

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

/* A workgroup loops over the 3 P point coordinates, then over the 3 V target coordinates, and sends once: the counts of
 * those that are not finite and, of the finite target coordinates, the box. */
__global__ __launch_bounds__(256) void extentKernel(const float *points, uint64_t numPointCoordinates, const float *vertices,
                                                    uint64_t numVertexCoordinates, Counter *counters)
{
    __shared__ GroupCounts<2, 6> totals;
    totals.clear();
    const int at[8] = {C_BAD_POINTS, C_BAD_VERTICES, C_BOX_MAX, C_BOX_MAX + 1, C_BOX_MAX + 2, C_BOX_MIN, C_BOX_MIN + 1, C_BOX_MIN + 2};
    const uint64_t first = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t) gridDim.x * blockDim.x;
    uint32_t badPoints = 0, badVertices = 0;
    for (uint64_t i = first; i < numPointCoordinates; i += stride)
        badPoints += isfinite(points[i]) ? 0u : 1u;
    /* the smallest is kept as the largest of the complements, which GroupCounts' maxima hold; 0 = none seen (the ordered bits
     * of a finite float are neither 0 nor all ones) */
    uint32_t most[3] = {0, 0, 0}, least[3] = {0, 0, 0};
    for (uint64_t i = first; i < numVertexCoordinates; i += stride)
    {
        const float x = vertices[i];
        const bool ok = isfinite(x);
        badVertices += ok ? 0u : 1u;
        const uint32_t o = orderedBits(__float_as_uint(x)), axis = (uint32_t) (i % 3);
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
            if (ok && axis == k)
            {
                most[k] = max(most[k], o);
                least[k] = max(least[k], ~o);
            }
    }
    totals.add(0, badPoints);
    totals.add(1, badVertices);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        totals.raise(k, most[k]);
        totals.raise(3 + k, least[k]);
    }
    totals.flush(counters, at);
}

/* Step 1, and the sum of the extents (the longest side of a live triangle's box, as a fraction of `scale`'s unit) that sizes
 * the first cell.  A workgroup loops and sends once; the extents go through one 64-bit atomic per wave. */
__global__ __launch_bounds__(256) void classifyKernel(const float *vertices, uint64_t numVertices, const uint32_t *tri, uint64_t numTriangles,
                                                      double scale, Counter *counters)
{
    __shared__ GroupCounts<3> totals;
    totals.clear();
    const int at[3] = {C_OUT_OF_RANGE, C_DEGENERATE, C_LIVE};
    uint32_t outOfRange = 0, degenerate = 0, live = 0;
    long long extents = 0;
    for (uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; t < numTriangles; t += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
        const TriangleDefect d = defectOf(i, numVertices);
        outOfRange += d.outOfRange ? 1u : 0u;
        degenerate += d.degenerate ? 1u : 0u;
        if (!d.none())
            continue;
        live++;
        const Corners T = cornersOf(vertices, tri, t);
        double extent = 0.0;
#pragma unroll
        for (int x = 0; x < 3; x++)
        {
            double from, to;
            reachOf(T, x, 0.0, &from, &to);
            extent = fmax(extent, to - from);
        }
        extents += (long long) fmin(extent * scale, (double) (1u << (EXTENT_BITS + 1)));
    }
    totals.add(0, outOfRange);
    totals.add(1, degenerate);
    totals.add(2, live);
    const long long ofWave = waveSum64(extents);
    if (laneId() == 0 && ofWave != 0)
        atomicAdd(&counters[C_EXTENT], (Counter) ofWave);
    totals.flush(counters, at);
}

/* the cells of triangle t per axis, first and last; false for a triangle that takes no part */
__device__ __forceinline__ bool cellsOf(const Grid &G, const float *vertices, uint64_t numVertices, const uint32_t *tri, uint64_t t,
                                        uint32_t first[3], uint32_t last[3])
{
    const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    if (!defectOf(i, numVertices).none())
        return false;
    const Corners T = cornersOf(vertices, tri, t);
#pragma unroll
    for (int x = 0; x < 3; x++)
    {
        double from, to;
        reachOf(T, x, G.D, &from, &to);
        first[x] = G.cell(x, from);
        last[x] = G.cell(x, to);
    }
    return true;
}

/* How many cells every triangle goes into: at most CELL_CAP^3 = 2^63, kept up to 2^32 (which is beyond every budget).  The
 * total goes through one 64-bit atomic per wave.  Every lane stays to the end. */
__global__ __launch_bounds__(256) void countKernel(Grid G, const float *vertices, uint64_t numVertices, const uint32_t *tri,
                                                   uint64_t numTriangles, uint32_t *counts, Counter *counters)
{
    long long pairs = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < numTriangles; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t t = base + threadIdx.x;
        if (t >= numTriangles)
            continue;
        uint32_t first[3], last[3];
        uint64_t cells = 0;
        if (cellsOf(G, vertices, numVertices, tri, t, first, last))
            cells = (uint64_t) (last[0] - first[0] + 1) * (last[1] - first[1] + 1) * (last[2] - first[2] + 1);
        cells = min(cells, (uint64_t) 1 << 32);
        counts[t] = (uint32_t) min(cells, (uint64_t) 0xFFFFFFFFu);
        pairs += (long long) cells;
    }
    const long long ofWave = waveSum64(pairs);
    if (laneId() == 0 && ofWave != 0)
        atomicAdd(&counters[C_PAIRS], (Counter) ofWave);
}

/* The pairs of triangle t, from starts[t] on: counts that passed the budget, so starts[t] + count <= numPairs.  The bound is
 * checked all the same: no store depends on the two kernels agreeing. */
__global__ __launch_bounds__(256) void emitKernel(Grid G, const float *vertices, uint64_t numVertices, const uint32_t *tri,
                                                  uint64_t numTriangles, const uint32_t *starts, uint64_t numPairs, uint64_t *keys,
                                                  uint32_t *vals)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    uint32_t first[3], last[3];
    if (!cellsOf(G, vertices, numVertices, tri, t, first, last))
        return;
    uint64_t at = starts[t];
    for (uint32_t z = first[2]; z <= last[2]; z++)
        for (uint32_t y = first[1]; y <= last[1]; y++)
            for (uint32_t x = first[0]; x <= last[0]; x++, at++)
                if (at < numPairs)
                {
                    keys[at] = G.key(x, y, z);
                    vals[at] = (uint32_t) t;
                }
}

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

/* the grid of cell size h over [lo, hi] per axis, or false if an axis would need more than CELL_CAP cells */
bool layGrid(const double lo[3], const double hi[3], double h, double D, Grid *G)
{
    G->h = h;
    G->D = D;
    uint32_t bits[3];
    for (int x = 0; x < 3; x++)
    {
        G->origin[x] = lo[x];
        const double cells = std::floor((hi[x] - lo[x]) / h) + 1.0;
        if (!(cells <= (double) CELL_CAP))
            return false;
        G->n[x] = (uint32_t) std::max(cells, 1.0);
        bits[x] = bitLength(G->n[x] - 1);
    }
    G->shiftY = bits[0];
    G->shiftZ = bits[0] + bits[1];
    return true;
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
    DeviceArray<Counter> counters;
    Counter h[C_WORDS];
    std::memset(h, 0, sizeof(h));
    PROPAGATE(counters.alloc(C_WORDS));
    HIP_CHECK(hipMemsetAsync(counters.get(), 0, C_WORDS * sizeof(Counter), ctx->stream));
    HIP_CHECK(hipMemsetAsync(&counters.get()[C_FARTHEST], 0xFF, sizeof(Counter), ctx->stream));         /* a minimum */
    const auto readBack = [&]() -> int {
        HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MLSGPU_OK;
    };

    if (np > 0 || nv > 0)
    {
        LAUNCH(ctx, "kernel.deviation.extent", extentKernel, dim3(std::min(divUp(3 * std::max(np, nv), 256), LOOP_BLOCKS)), B, dPoints, 3 * np,
               dVertices, 3 * nv, counters.get());
        PROPAGATE(readBack());
    }
    if (h[C_BAD_POINTS] != 0 || h[C_BAD_VERTICES] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh deviation: %llu point and %llu target coordinates are not finite", h[C_BAD_POINTS],
                        h[C_BAD_VERTICES]);

    /* the target's box, inflated by D (no finite coordinate lies outside; without vertices there is no triangle to bin) */
    double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, side = 0.0;
    if (nv > 0)
        for (int x = 0; x < 3; x++)
        {
            const double least = (double) fromOrdered(~(uint32_t) h[C_BOX_MIN + x]), most = (double) fromOrdered((uint32_t) h[C_BOX_MAX + x]);
            side = std::max(side, most - least);
            lo[x] = least - D;
            hi[x] = most + D;
        }

    /* a triangle's extent is summed in units of 2^-EXTENT_BITS of the power of two above the box's longest side */
    uint64_t bitsOfSide;
    std::memcpy(&bitsOfSide, &side, sizeof(side));
    const int eSide = side > 0.0 ? exponentOfDoubleBits(bitsOfSide) + 1 : 0;
    if (nv > 0 && nt > 0)
    {
        LAUNCH(ctx, "kernel.deviation.classify", classifyKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, dVertices, nv, dTriangles, nt,
               powerOfTwo((int) EXTENT_BITS - eSide), counters.get());
        PROPAGATE(readBack());
        out->outOfRangeTriangles = h[C_OUT_OF_RANGE];
        out->degenerateTriangles = h[C_DEGENERATE];
    }
    else
        out->outOfRangeTriangles = nt;          /* every index is >= 0 vertices */
    const uint64_t live = h[C_LIVE];
    if (np == 0)
        return MLSGPU_OK;

    DeviceArray<double> ownDistance2;
    if (dDistance2 == nullptr)
    {
        PROPAGATE(ownDistance2.alloc(np));
        dDistance2 = ownDistance2.get();
    }
    double scratch = (double) (counters.bytes(C_WORDS) + (ownDistance2.get() != nullptr ? ownDistance2.bytes(np) : 0));
    SortScratch pairs, sortedPoints;
    DeviceArray<uint32_t> counts, starts, tileSums;
    if (live == 0)
        LAUNCH(ctx, "kernel.deviation.distance", beyondKernel, dim3(divUp(np, 256)), B, np, dDistance2, dNearest);
    else
    {
        PROPAGATE(counts.alloc(nt));
        PROPAGATE(starts.alloc(nt));
        PROPAGATE(tileSums.alloc((uint64_t) scanTiles(nt) + 1));
        PROPAGATE(sortedPoints.alloc(np));
        /* the first cell: twice D, or the mean extent of a triangle where that is larger; then doubled until every axis has
         * at most CELL_CAP cells and the pairs fit their budget.  One cell holds every live triangle once: the loop ends. */
        const uint64_t budget = std::max(MIN_PAIR_BUDGET, (uint64_t) PAIRS_PER_TRIANGLE * live);
        const double meanExtent = (double) h[C_EXTENT] / (double) live * powerOfTwo(eSide - (int) EXTENT_BITS);
        double cellSize = std::max(2.0 * D, meanExtent);
        Grid G;
        uint64_t numPairs = 0;
        for (;; cellSize *= 2.0)
        {
            if (!std::isfinite(cellSize))
                return setError(MLSGPU_ERR_LENGTH, "mesh deviation: no cell size brings the grid's pairs under %llu",
                                (unsigned long long) budget);
            if (!layGrid(lo, hi, cellSize, D, &G))
                continue;
            HIP_CHECK(hipMemsetAsync(&counters.get()[C_PAIRS], 0, sizeof(Counter), ctx->stream));
            LAUNCH(ctx, "kernel.deviation.count", countKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, G, dVertices, nv, dTriangles, nt,
                   counts.get(), counters.get());
            PROPAGATE(readBack());
            numPairs = h[C_PAIRS];
            if (numPairs <= budget)
                break;
        }
        REQUIRE(numPairs >= live && numPairs < (uint64_t(1) << 32), MLSGPU_ERR_LENGTH);
        PROPAGATE(pairs.alloc(numPairs));
        scratch += (double) (pairs.bytes() + sortedPoints.bytes() + 2 * counts.bytes(nt) + tileSums.bytes((uint64_t) scanTiles(nt) + 1));
        if (ctx->timing)
        {
            ctx->addValue("deviation.pairs", (double) numPairs);
            ctx->addValue("deviation.cellsize", cellSize);
        }

        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.deviation.scan", ArrayIn<uint32_t>{counts.get()}, ArrayOut<uint32_t>{starts.get()}, nt,
                                           0u, tileSums.get(), (uint32_t *) nullptr)));
        LAUNCH(ctx, "kernel.deviation.emit", emitKernel, dim3(divUp(nt, 256)), B, G, dVertices, nv, dTriangles, nt,
               (const uint32_t *) starts.get(), numPairs, pairs.keys(), pairs.vals());
        /* (both sorts under one name: a launch site of the sort keeps one stat id per translation unit) */
        const uint32_t keyBits = G.shiftZ + bitLength(G.n[2] - 1);
        SortResult<uint64_t> byCell = {nullptr, nullptr}, pointsByCell = {nullptr, nullptr};
        PROPAGATE(radixSort<uint64_t>(ctx, "kernel.deviation.sort", pairs.keysA, pairs.valsA, pairs.keysB, pairs.valsB, numPairs, keyBits,
                                      false, pairs.hist, nullptr, &byCell));
        LAUNCH(ctx, "kernel.deviation.pointkeys", pointKeysKernel, dim3(divUp(np, 256)), B, G, dPoints, np, sortedPoints.keys());
        PROPAGATE(radixSort<uint64_t>(ctx, "kernel.deviation.sort", sortedPoints.keysA, sortedPoints.valsA, sortedPoints.keysB,
                                      sortedPoints.valsB, np, keyBits, true, sortedPoints.hist, nullptr, &pointsByCell));
        /* lanes per point: a power of two, as many as keep the launch under SPREAD_THREADS lanes.  (MLSGPU_HIP_DEVIATION_LANES
         * is a tuning aid; the result does not depend on it.) */
        uint32_t laneShift = 0;
        while (laneShift < 6 && (np << (laneShift + 1)) <= SPREAD_THREADS)
            laneShift++;
        if (const char *forced = getenv("MLSGPU_HIP_DEVIATION_LANES"))
        {
            const int lanes = atoi(forced);
            if (lanes >= 1 && lanes <= WAVE_LANES && (lanes & (lanes - 1)) == 0)
                laneShift = bitLength((uint64_t) lanes) - 1;
        }
        if (ctx->timing)
            ctx->addValue("deviation.lanes", (double) (1u << laneShift));
        LAUNCH(ctx, "kernel.deviation.distance", distanceKernel, dim3(divUp(np << laneShift, 256)), B, dPoints,
               (const uint64_t *) pointsByCell.keys, (const uint32_t *) pointsByCell.vals, np, laneShift, dVertices, dTriangles, (const uint64_t *) byCell.keys, (const uint32_t *) byCell.vals,
               (uint32_t) numPairs, D, dDistance2, dNearest, ctx->timing ? &counters.get()[C_HANDED] : (Counter *) nullptr);
    }
    if (ctx->timing)
        ctx->addValue("deviation.scratch.bytes", scratch);

    LAUNCH(ctx, "kernel.deviation.report", reportKernel, dim3(std::min(divUp(np, 256), LOOP_BLOCKS)), B, (const double *) dDistance2, np, D2,
           powerOfTwo(30 - e), counters.get());
    LAUNCH(ctx, "kernel.deviation.report", farthestKernel, dim3(divUp(np, 256)), B, (const double *) dDistance2, np, counters.get());
    PROPAGATE(readBack());      /* the scratch goes with the call */
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
