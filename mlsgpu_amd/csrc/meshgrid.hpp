/*
 * The sparse uniform grid over a mesh's triangles that the deviation report (deviation.hip) and the self-intersection report
 * (intersect.hip) are built on: the (cell key, triangle) records of every triangle that takes part, sorted by cell.  What the
 * stages do with the cells' runs is theirs; how the grid is made is here, and its host arithmetic in meshgridplan.hpp.
 *
 *   extent     over the coordinates of the points (if any) and of the vertices: those that are not finite, and the box of
 *              the finite vertex coordinates                                                          -- one read-back --
 *   classify   over the triangles: which take no part, and the fixed-point sum of the bounding-box extents of the others,
 *              whose mean sizes the first cell                                                        -- one read-back --
 *   count      a thread per triangle: the cells its box, inflated by `reach`, touches.  The host doubles the cell size and
 *              counts again until the records fit their budget                              -- one read-back per size --
 *   emit       a scan over the counts, then a thread per triangle writes its (cell key, triangle) records
 *   sort       the records by cell key
 *
 * Four facts both stages' arguments rest on.  cell(x) = clamp(floor((x - origin) / h), 0, n - 1) is three correctly rounded,
 * monotone steps, hence monotone in x, and clamped to the grid.  A triangle goes into every cell from cell(lo - reach) to
 * cell(hi + reach) per axis, lo and hi its box's float corners widened: the SAME rounded doubles its user compares with
 * (x - 0.0 == x and x + 0.0 == x for every double, so a reach of 0.0 bins lo and hi themselves).  An index >= V is compared
 * and counted, never used as an address, and no address depends on a coordinate except through cell().  emit checks every
 * store against the number of records even though count sized them: no store depends on two kernels agreeing.
 *
 * A stage's counter block begins with the grid's words (G_WORDS of them); the stage's own follow.
 */
#ifndef MLSGPU_AMD_MESHGRID_HPP
#define MLSGPU_AMD_MESHGRID_HPP

#include "meshgridplan.hpp"
#include "meshpost.hpp"

#include <initializer_list>
#include <vector>

namespace mlsgpu
{

enum
{
    G_BAD_VERTICES = 0,         /* vertex coordinates that are not finite */
    G_OUT_OF_RANGE = 1,
    G_DEGENERATE = 2,
    G_LIVE = 3,                 /* triangles that take part */
    G_EXTENT = 4,               /* the fixed-point sum of their extents */
    G_RECORDS = 5,              /* the records of the last count */
    G_BOX_MIN = 6,              /* 3: the smallest vertex coordinate per axis, as ordered bits (complemented) */
    G_BOX_MAX = 9,              /* 3: the largest */
    G_WORDS = 12
};

/* per axis the smallest and the largest coordinate of the corners i[0 .. 2], indices known to be in range */
struct TriangleBox
{
    float lo[3], hi[3];
};
__device__ __forceinline__ TriangleBox triangleBox(const float *vertices, const uint64_t i[3])
{
    TriangleBox B;
#pragma unroll
    for (int x = 0; x < 3; x++)
    {
        const float a = vertices[3 * i[0] + x], b = vertices[3 * i[1] + x], c = vertices[3 * i[2] + x];
        B.lo[x] = fminf(fminf(a, b), c);
        B.hi[x] = fmaxf(fmaxf(a, b), c);
    }
    return B;
}

namespace       /* as meshpost.hpp's: a launch site keeps its stat id per translation unit, and a stage has one set of names */
{

/* A workgroup loops over the point coordinates (none without points), then over the 3 V vertex coordinates, and sends once:
 * the counts of those that are not finite -- the points' to counters[badPointsAt], a word of the stage's own that is never
 * sent without points -- and, of the finite vertex coordinates, the box. */
__global__ __launch_bounds__(256) void extentKernel(const float *points, uint64_t numPointCoordinates, const float *vertices,
                                                    uint64_t numVertexCoordinates, int badPointsAt, Counter *counters)
{
    __shared__ GroupCounts<2, 6> totals;
    totals.clear();
    const int at[8] = {badPointsAt, G_BAD_VERTICES, G_BOX_MAX, G_BOX_MAX + 1, G_BOX_MAX + 2, G_BOX_MIN, G_BOX_MIN + 1, G_BOX_MIN + 2};
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

/* Which triangles take no part, and the sum of the extents (the longest side of a live triangle's box, as a fraction of
 * `scale`'s unit) that sizes the first cell.  A workgroup loops and sends once; the extents go through one 64-bit atomic per
 * wave. */
__global__ __launch_bounds__(256) void classifyKernel(const float *vertices, uint64_t numVertices, const uint32_t *tri, uint64_t numTriangles,
                                                      double scale, Counter *counters)
{
    __shared__ GroupCounts<3> totals;
    totals.clear();
    const int at[3] = {G_OUT_OF_RANGE, G_DEGENERATE, G_LIVE};
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
        const TriangleBox B = triangleBox(vertices, i);
        double extent = 0.0;
#pragma unroll
        for (int x = 0; x < 3; x++)
            extent = fmax(extent, (double) B.hi[x] - (double) B.lo[x]);
        extents += (long long) fmin(extent * scale, (double) (1u << (EXTENT_BITS + 1)));
    }
    totals.add(0, outOfRange);
    totals.add(1, degenerate);
    totals.add(2, live);
    const long long ofWave = waveSum64(extents);
    if (laneId() == 0 && ofWave != 0)
        atomicAdd(&counters[G_EXTENT], (Counter) ofWave);
    totals.flush(counters, at);
}

/* the cells of triangle t per axis, first and last; false for a triangle that takes no part */
__device__ __forceinline__ bool cellsOf(const Grid &G, const float *vertices, uint64_t numVertices, const uint32_t *tri, uint64_t t,
                                        uint32_t first[3], uint32_t last[3])
{
    const uint64_t i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    if (!defectOf(i, numVertices).none())
        return false;
    const TriangleBox B = triangleBox(vertices, i);
#pragma unroll
    for (int x = 0; x < 3; x++)
    {
        first[x] = G.cell(x, (double) B.lo[x] - G.reach);
        last[x] = G.cell(x, (double) B.hi[x] + G.reach);
    }
    return true;
}

/* How many cells every triangle goes into: at most CELL_CAP^3 = 2^63, kept up to 2^32 (which is beyond every budget); and,
 * where lowerCell is taken, the cell of its box's lower corner, packed.  The total goes through one 64-bit atomic per wave.
 * Every lane stays to the end. */
__global__ __launch_bounds__(256) void countKernel(Grid G, const float *vertices, uint64_t numVertices, const uint32_t *tri,
                                                   uint64_t numTriangles, uint32_t *counts, uint64_t *lowerCell, Counter *counters)
{
    long long records = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < numTriangles; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t t = base + threadIdx.x;
        if (t >= numTriangles)
            continue;
        uint32_t first[3] = {0, 0, 0}, last[3] = {0, 0, 0};
        uint64_t cells = 0;
        if (cellsOf(G, vertices, numVertices, tri, t, first, last))
            cells = (uint64_t) (last[0] - first[0] + 1) * (last[1] - first[1] + 1) * (last[2] - first[2] + 1);
        cells = min(cells, (uint64_t) 1 << 32);
        counts[t] = (uint32_t) min(cells, (uint64_t) 0xFFFFFFFFu);
        if (lowerCell != nullptr)
            lowerCell[t] = packCell(first[0], first[1], first[2]);
        records += (long long) cells;
    }
    const long long ofWave = waveSum64(records);
    if (laneId() == 0 && ofWave != 0)
        atomicAdd(&counters[G_RECORDS], (Counter) ofWave);
}

/* The records of triangle t, from starts[t] on: counts that passed the budget, so starts[t] + count <= numRecords.  The bound
 * is checked all the same. */
__global__ __launch_bounds__(256) void emitKernel(Grid G, const float *vertices, uint64_t numVertices, const uint32_t *tri,
                                                  uint64_t numTriangles, const uint32_t *starts, uint64_t numRecords, uint64_t *keys,
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
                if (at < numRecords)
                {
                    keys[at] = G.key(x, y, z);
                    vals[at] = (uint32_t) t;
                }
}

/* ---------------------------------------------------------------- the driver (host) */

/* A stage's counter block on the device and its copy on the host. */
struct CounterBlock
{
    DeviceArray<Counter> device;
    std::vector<Counter> h;     /* what the last readBack() found */

    /* `words` zeros, but all ones in the words that hold a minimum */
    int start(mlsgpu_ctx *ctx, uint32_t words, std::initializer_list<int> minima)
    {
        h.assign(words, 0);
        PROPAGATE(device.alloc(words));
        HIP_CHECK(hipMemsetAsync(device.get(), 0, words * sizeof(Counter), ctx->stream));
        for (int word : minima)
            HIP_CHECK(hipMemsetAsync(&device.get()[word], 0xFF, sizeof(Counter), ctx->stream));
        return MLSGPU_OK;
    }
    /* the whole block, and the stream idle */
    int readBack(mlsgpu_ctx *ctx)
    {
        HIP_CHECK(hipMemcpyAsync(h.data(), device.get(), h.size() * sizeof(Counter), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MLSGPU_OK;
    }
    Counter *get() const { return device.get(); }
    uint64_t bytes() const { return device.bytes(h.size()); }
};

/* what a stage calls the grid's launches, statistics and records */
struct GridNames
{
    const char *stage, *records;        /* for the error texts: "mesh deviation", "pairs" */
    const char *extent, *classify, *count, *scan, *emit, *sort;
    const char *numRecords, *cellSize;
};

/* The grid of one call, in two steps; between them the stage takes its own early exits. */
struct TriangleGrid
{
    mlsgpu_ctx *ctx;
    const GridNames &names;
    CounterBlock &counters;
    const float *vertices;
    uint64_t nv;
    const uint32_t *tri;
    uint64_t nt;
    double reach;

    /* behind measure() */
    uint64_t badPoints = 0, badVertices = 0, outOfRange = 0, degenerate = 0, live = 0, extentSum = 0;
    GridBox box;
    /* behind build() */
    Grid G;
    double cellSize = 0.0;
    uint64_t numRecords = 0;
    SortResult<uint64_t> byCell = {nullptr, nullptr};   /* the records by cell key, their triangles along */
    DeviceArray<uint32_t> counts, starts, tileSums;
    SortScratch records;

    /* extent, then -- unless a coordinate is not finite, which the stage refuses in its own words -- classify */
    int measure(const float *points, uint64_t np, int badPointsAt)
    {
        const dim3 B(256);
        if (np > 0 || nv > 0)
        {
            LAUNCH(ctx, names.extent, extentKernel, dim3(std::min(divUp(3 * std::max(np, nv), 256), LOOP_BLOCKS)), B, points, 3 * np,
                   vertices, 3 * nv, badPointsAt, counters.get());
            PROPAGATE(counters.readBack(ctx));
        }
        const std::vector<Counter> &h = counters.h;
        badPoints = np > 0 ? h[badPointsAt] : 0;
        badVertices = h[G_BAD_VERTICES];
        if (badPoints != 0 || badVertices != 0)
            return MLSGPU_OK;
        box = boxOfWords(&h[G_BOX_MIN], &h[G_BOX_MAX], nv > 0, reach);
        if (nv > 0 && nt > 0)
        {
            LAUNCH(ctx, names.classify, classifyKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, vertices, nv, tri, nt,
                   powerOfTwo((int) EXTENT_BITS - box.eSide), counters.get());
            PROPAGATE(counters.readBack(ctx));
            outOfRange = h[G_OUT_OF_RANGE];
            degenerate = h[G_DEGENERATE];
        }
        else
            outOfRange = nt;            /* every index is >= 0 vertices */
        live = h[G_LIVE];
        extentSum = h[G_EXTENT];
        return MLSGPU_OK;
    }

    /* the size the doubling starts from (live > 0) */
    double firstCell() const { return firstCellSize(extentSum, live, box.eSide, box.side, reach); }

    /* The cell size from firstCell on, doubled until every axis has at most CELL_CAP cells and the records fit their budget
     * (one cell holds every live triangle once: the loop ends); then the records, sorted.  live > 0. */
    int build(double firstCell, uint64_t *lowerCell)
    {
        const dim3 B(256);
        PROPAGATE(counts.alloc(nt));
        PROPAGATE(starts.alloc(nt));
        PROPAGATE(tileSums.alloc((uint64_t) scanTiles(nt) + 1));
        const uint64_t budget = recordBudget(live);
        for (cellSize = firstCell;; cellSize *= 2.0)
        {
            if (!std::isfinite(cellSize))
                return setError(MLSGPU_ERR_LENGTH, "%s: no cell size brings the grid's %s under %llu", names.stage, names.records,
                                (unsigned long long) budget);
            if (!layGrid(box.lo, box.hi, cellSize, reach, &G))
                continue;
            HIP_CHECK(hipMemsetAsync(&counters.get()[G_RECORDS], 0, sizeof(Counter), ctx->stream));
            LAUNCH(ctx, names.count, countKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, G, vertices, nv, tri, nt, counts.get(),
                   lowerCell, counters.get());
            PROPAGATE(counters.readBack(ctx));
            numRecords = counters.h[G_RECORDS];
            if (numRecords <= budget)
                break;
        }
        REQUIRE(numRecords >= live && numRecords < (uint64_t(1) << 32), MLSGPU_ERR_LENGTH);
        PROPAGATE(records.alloc(numRecords));
        if (ctx->timing)
        {
            ctx->addValue(names.numRecords, (double) numRecords);
            ctx->addValue(names.cellSize, cellSize);
        }
        PROPAGATE((exclusiveScan<uint32_t>(ctx, names.scan, ArrayIn<uint32_t>{counts.get()}, ArrayOut<uint32_t>{starts.get()}, nt, 0u,
                                           tileSums.get(), (uint32_t *) nullptr)));
        LAUNCH(ctx, names.emit, emitKernel, dim3(divUp(nt, 256)), B, G, vertices, nv, tri, nt, (const uint32_t *) starts.get(), numRecords,
               records.keys(), records.vals());
        return radixSort<uint64_t>(ctx, names.sort, records.keysA, records.valsA, records.keysB, records.valsB, numRecords, G.keyBits(),
                                   false, records.hist, nullptr, &byCell);
    }

    /* the scratch of build() */
    uint64_t bytes() const { return records.bytes() + 2 * counts.bytes(nt) + tileSums.bytes((uint64_t) scanTiles(nt) + 1); }
};

} // namespace

} // namespace mlsgpu

#endif
