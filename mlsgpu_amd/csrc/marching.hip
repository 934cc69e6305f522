/*
 * Marching tetrahedra with on-device welding on gfx950 -- the device half of Marching
 * (reference: src/marching.{h,cpp}, kernels/marching.cl) plus ScaleBiasFilter
 * (src/mesh_filter.cpp:69-113, kernels/scale_bias.cl) and enqueueReadMesh (src/mesh.cpp:62-102).
 *
 * Data contracts kept from the reference: lookup tables (makeTables), vertex-key bit layout,
 * external-vertex rule, internal-first / external-last output order, DeviceKeyMesh layout, the
 * swathe loop and the mesh-memory overflow protocol of addSlices / shipOut.
 *
 * Mechanism, MI355X-first:
 *  - the distance field is a plain HBM buffer addressed like the reference's packed 2-D image
 *    (CDNA has no image path); with no 8192-row image limit a swathe may span the whole bucket;
 *  - a bucket that one swathe spans is welded without a sort, from the half lattice of the resident field (the lattice
 *    weld); any other goes through the reference's generate + sort + compact structure (the sort weld);
 *  - host synchronisations per bucket: one per swathe (totals) + one per ship-out (welded sizes).
 *
 * This file is the host object: the buffers, the generate protocol (swathe loop, addSlices, shipOut), the C API and the
 * mesh plumbing.  The one translation unit is made of four more files, which nothing else includes:
 *   marchingplan.hpp      the host arithmetic, without HIP: buffer sizes, lattice geometry and launch counts, the rules
 *                         that pick a weld, a mask kernel and a triangle route, key layout, slice runs of an overflow
 *   marching_tables.hpp   makeTables and the tables derived from it
 *   marching_sort.hpp     cell classification (both welds) and the sort weld's kernels
 *   marching_lattice.hpp  the lattice weld's kernels
 */
#include "common.hpp"
#include <type_traits>
#include "primitives.hpp"
#include "marchingplan.hpp"
#include "marching_tables.hpp"
#include "marching_sort.hpp"
#include "marching_lattice.hpp"

#include <algorithm>
#include <cassert>
#include <cstdlib>

using namespace mlsgpu;

namespace
{

/* copySlice, kernels/marching.cl:349-358 / clEnqueueCopyImage in src/marching.cpp:447-498 */
__global__ __launch_bounds__(256) void copySliceKernel(float *field, uint64_t pitch, uint32_t srcRow, uint32_t trgRow,
                                                       uint32_t width, uint32_t height)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < width * height)
    {
        const uint32_t x = i % width, y = i / width;
        field[(uint64_t) (trgRow + y) * pitch + x] = field[(uint64_t) (srcRow + y) * pitch + x];
    }
}

/* scaleBiasVertices, kernels/scale_bias.cl:33-41 */
__global__ __launch_bounds__(256) void scaleBiasKernel(float *vertices, uint64_t numFloats, float scale,
                                                       float bx, float by, float bz)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < numFloats)
    {
        const uint32_t axis = (uint32_t) (i % 3);
        const float b = axis == 0 ? bx : (axis == 1 ? by : bz);
        vertices[i] = fmaf(vertices[i], scale, b);
    }
}

/* device words the host waits for; it reads them from the mailbox, except shipOutSorted's two through hReadback */
struct Readback
{
    U3 totals;              /* occupied cells, vertices, indices of the (sub-)swathe */
    uint32_t numWelded;
    uint32_t firstExternal;
    U3 classTotals;         /* lattice weld: welded vertices per class (internal, unflagged top, flagged) */
    U3 batchTotals;         /* lattice weld: occupied cells / vertices / indices of the batch */
};

/* ... as they lie in device memory, with the two words behind them that are no read-back */
struct ReadbackWords : Readback
{
    uint32_t idle[16];      /* [0]: the word latticeTrianglesRowKernel's idle stores hit */
    uint32_t gate[16];      /* [0]: the gate of rowTotalsKernel (zero between launches) */
};
static_assert(sizeof(ReadbackWords) == sizeof(Readback) + 128, "the words lie right behind the read-back");

} // namespace

struct mlsgpu_marching : MarchingSizes     /* imageWidth .. latWords: what follows from the constructor's arguments */
{
    mlsgpu_ctx *ctx = nullptr;
    uint32_t maxWidth = 0, maxHeight = 0, maxDepth = 0;
    bool wideKeys = false;
    HostTables tables;

    DeviceArray<float> dField;
    DeviceArray<uchar2> dCount;
    DeviceArray<ushort2> dStart;
    DeviceArray<uint8_t> dData;
    DeviceArray<uint32_t> dKey;
    DeviceArray<uint32_t> dCodeRec;
    DeviceArray<uint64_t> dEdgeLut;         /* makeEdgeLut */
    DeviceArray<uint16_t> dEdgeLut16;       /* makeEdgeLut16 */
    DeviceArray<uint2> dCells, dViStart, dHistogram;
    DeviceArray<U3> dTileSums3;
    DeviceArray<float4> dVertices;
    DeviceArray<uint64_t> dKeysA, dKeysB;   /* 32-bit keys when !wideKeys */
    DeviceArray<uint32_t> dValsA, dValsB;
    DeviceArray<uint32_t> dIndices, dIndexRemap;
    DeviceArray<float> dWelded;             /* 3 per vertex */
    DeviceArray<uint64_t> dWeldedKeys;
    DeviceArray<uint32_t> dHist, dTileSums;
    DeviceArray<ReadbackWords> dReadback;   /* device words */
    PinnedArray<Readback> hReadback;        /* numWelded / firstExternal of shipOutSorted */
    HostMailbox box;                        /* the totals a host decision waits for (swathe totals, welded counts) */
    PinnedArray<uint2> hHistogram;          /* maxDepth entries (viReadback in the reference) */

    /* lattice weld (single-swathe buckets) */
    DeviceArray<uint8_t> dCellCode;
    DeviceArray<U3> dRowCounts, dRowStarts; /* per row of cells of the swathe: (occupied, vertices, indices) */
    DeviceArray<LatWord> dLatWords;
    DeviceArray<U3> dLatRows;

    uint64_t counters[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    VertexTransform transform = {1.0f, 0.0f, 0.0f, 0.0f, 0};

    /* per-generate state */
    bool direct = false;                    /* this generate() call uses the lattice weld */
    uint32_t codeZ0 = 0;                    /* first cell slice held in dCellCode */
    uint32_t bufferedCells = 0;             /* occupied cells accounted since the last ship-out (direct mode) */
    uint32_t offsets[2] = {0, 0};           /* vertices / indices accounted since the last ship-out */
    uint32_t zTop = 0;                      /* first cell slice of what is buffered */
    uint64_t shipOutsBefore = 0;            /* counters[1] when the call began */
    mlsgpu_batch_output_fn output = nullptr;
    void *outputUser = nullptr;
    uint32_t outputIndex = 0;               /* the bucket's index in the call */
    uint32_t keyOffset[3] = {0, 0, 0};
    KeyLayout layout = {1, 1, 1};

    mlsgpu_marching(uint32_t maxWidth, uint32_t maxHeight, uint32_t maxDepth, uint32_t swatheLimit, uint64_t meshMemory,
                    const uint32_t alignment[3])
        : MarchingSizes(maxWidth, maxHeight, maxDepth, swatheLimit, meshMemory, alignment), maxWidth(maxWidth),
          maxHeight(maxHeight), maxDepth(maxDepth)
    {
    }
    ~mlsgpu_marching() { box.destroy(); }

    /* Every device buffer with its element count, once: each(array, elements) until one fails.
     * mlsgpu_hip_marching_create allocates them, mlsgpu_hip_marching_resource_usage adds them up. */
    template<typename Each>
    int buffers(Each each)
    {
        const uint64_t vs = vertexSpace, sc = swatheCells, cellRows = (uint64_t) maxSwathe * (maxHeight - 1);
        PROPAGATE(each(dField, fieldRows * imageWidth));
        PROPAGATE(each(dCount, 256));
        PROPAGATE(each(dStart, 257));
        PROPAGATE(each(dData, 8192));
        PROPAGATE(each(dKey, 2432));
        PROPAGATE(each(dCodeRec, 256 * 16));
        PROPAGATE(each(dEdgeLut, 256));
        PROPAGATE(each(dEdgeLut16, 4 * 256));
        PROPAGATE(each(dCells, sc));
        PROPAGATE(each(dViStart, sc));
        PROPAGATE(each(dHistogram, maxDepth));
        PROPAGATE(each(dTileSums3, (uint64_t) scanTiles(std::max(sc, latRowsMax)) + 1));
        PROPAGATE(each(dCellCode, sc + 64));        /* latticeMaskWordKernel reads whole 32-byte words: up to 31 bytes behind the last row */
        PROPAGATE(each(dRowCounts, cellRows + 1));
        PROPAGATE(each(dRowStarts, cellRows + 1));
        PROPAGATE(each(dLatWords, latRowsMax * latWords));
        PROPAGATE(each(dLatRows, latRowsMax));
        if (legacyBuffers)
        {
            PROPAGATE(each(dVertices, vs));         /* unwelded */
            PROPAGATE(each(dKeysA, vs + 1));        /* sort keys and values, ping-pong */
            PROPAGATE(each(dKeysB, vs + 1));
            PROPAGATE(each(dValsA, vs + 1));
            PROPAGATE(each(dValsB, vs + 1));
            PROPAGATE(each(dIndexRemap, vs));
            PROPAGATE(each(dHist, sortHistElems(vs) + 1));
            PROPAGATE(each(dTileSums, (uint64_t) scanTiles(std::max<uint64_t>(sortHistElems(vs), vs)) + 1));
        }
        PROPAGATE(each(dIndices, indexSpace));
        PROPAGATE(each(dWelded, vs * 3));
        PROPAGATE(each(dWeldedKeys, vs));
        PROPAGATE(each(dReadback, 1));
        return MLSGPU_OK;
    }

    FieldView view(const mlsgpu_swathe &sw) const { return FieldView{dField, imageWidth, sw.zStride, sw.zBias}; }
    CodeView codeView(const mlsgpu_swathe &sw) const { return CodeView{dCellCode, sw.width - 1, sw.height - 1, codeZ0}; }
    DevTables devTables() const { return DevTables{dCount, dStart, dData, dKey, dCodeRec}; }
    /* keyOffset as the vertex keys carry it (one fractional bit per axis), src/marching.cpp:594-597 */
    uint64_t packedKeyOffset() const
    {
        return ((uint64_t) keyOffset[2] << (2 * KEY_AXIS_BITS + 1)) | ((uint64_t) keyOffset[1] << (KEY_AXIS_BITS + 1))
            | ((uint64_t) keyOffset[0] << 1);
    }

    /* the mesh of a ship-out of numIndices indices, in the output buffers of either weld; the weld fills in the vertex counts */
    mlsgpu_mesh meshOf(uint32_t numIndices) const
    {
        mlsgpu_mesh mesh = mlsgpu_mesh();
        mesh.dVertices = dWelded;
        mesh.dTriangles = dIndices;
        mesh.dVertexKeys = dWeldedKeys;
        mesh.numTriangles = numIndices / 3;
        return mesh;
    }

    int generateCells(const mlsgpu_swathe &sw, U3 *totals);
    int sliceHistogram(const mlsgpu_swathe &sw);
    int computeCodes(const mlsgpu_swathe &sw);
    int shipOut(const mlsgpu_swathe &sw, uint32_t zMax);
    int shipOutSorted(uint32_t zMax, mlsgpu_mesh *mesh);
    int shipOutDone(const mlsgpu_mesh &mesh);
    CellCodeArgs cellCodeArgs(const mlsgpu_swathe &sw);
    bool overflows(const U3 &totals) const { return totals.b > vertexSpace || totals.c > indexSpace; }
    int addSlices(const mlsgpu_swathe &sw, const U3 &totals);
    int endGenerate(const mlsgpu_swathe &sw);
    template<typename K> int weld(uint32_t nv, uint32_t zMax);
};

MLSGPU_API uint64_t mlsgpu_hip_marching_resource_usage(uint32_t maxWidth, uint32_t maxHeight, uint32_t maxDepth,
                                                       uint32_t maxSwathe, uint64_t meshMemory, const uint32_t alignment[3])
{
    /* device memory only: the pinned read-backs and the mailbox are host memory */
    uint64_t bytes = 0;
    mlsgpu_marching(maxWidth, maxHeight, maxDepth, maxSwathe, meshMemory, alignment).buffers([&](auto &array, uint64_t n) {
        bytes += array.bytes(n);
        return MLSGPU_OK;
    });
    return bytes;
}

MLSGPU_API int mlsgpu_hip_marching_create(mlsgpu_ctx *ctx, uint32_t maxWidth, uint32_t maxHeight, uint32_t maxDepth,
                                          uint32_t maxSwathe, uint64_t meshMemory, const uint32_t alignment[3],
                                          mlsgpu_marching **out)
{
    REQUIRE(ctx != nullptr && out != nullptr && alignment != nullptr, MLSGPU_ERR_INVALID);
    /* src/marching.cpp:359-363 */
    REQUIRE(2 <= maxWidth && maxWidth <= MLSGPU_MARCHING_MAX_DIMENSION, MLSGPU_ERR_INVALID);
    REQUIRE(2 <= maxHeight && maxHeight <= MLSGPU_MARCHING_MAX_DIMENSION, MLSGPU_ERR_INVALID);
    REQUIRE(2 <= maxDepth && maxDepth <= MLSGPU_MARCHING_MAX_DIMENSION, MLSGPU_ERR_INVALID);
    REQUIRE(alignment[0] >= 1 && alignment[1] >= 1 && alignment[2] >= 1, MLSGPU_ERR_INVALID);
    REQUIRE(alignment[2] <= maxSwathe, MLSGPU_ERR_INVALID);
    REQUIRE(meshMemory >= (uint64_t) (maxWidth - 1) * (maxHeight - 1) * MLSGPU_MARCHING_MAX_CELL_BYTES, MLSGPU_ERR_INVALID);
    HIP_CHECK(hipSetDevice(ctx->device));

    std::unique_ptr<mlsgpu_marching> m(new mlsgpu_marching(maxWidth, maxHeight, maxDepth, maxSwathe, meshMemory, alignment));
    m->ctx = ctx;
    if (m->vertexSpace >= (uint64_t(1) << 32) || m->indexSpace >= (uint64_t(1) << 32))
        return setError(MLSGPU_ERR_LENGTH, "Marching: meshMemory gives more than 2^32 vertices or indices");
    if (m->swatheCells >= (uint64_t(1) << 32))
        return setError(MLSGPU_ERR_LENGTH, "Marching: more than 2^32 cells per swathe");
    makeTables(m->tables);
    assert(m->tables.data.size() == 8192 && m->tables.key.size() == 2432 * 3);    /* src/marching.cpp:248-251 */

    PROPAGATE(m->buffers([](auto &array, uint64_t n) { return array.alloc(n); }));
    HIP_CHECK(hipMemset(m->dReadback, 0, sizeof(ReadbackWords)));
    PROPAGATE(m->hReadback.alloc(1));
    PROPAGATE(m->hHistogram.alloc(maxDepth));
    PROPAGATE(m->box.create());
    /* upload the tables */
    const std::vector<uint32_t> packedKey = makePackedKeys(m->tables), codeRec = makeCodeRecords(m->tables);
    hipError_t e = hipMemcpy(m->dCount, m->tables.count, 512, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->dCodeRec, codeRec.data(), codeRec.size() * 4, hipMemcpyHostToDevice);
    const std::vector<uint64_t> edgeLut = makeEdgeLut();
    if (e == hipSuccess) e = hipMemcpy(m->dEdgeLut, edgeLut.data(), edgeLut.size() * 8, hipMemcpyHostToDevice);
    const std::vector<uint16_t> edgeLut16 = makeEdgeLut16();
    if (e == hipSuccess) e = hipMemcpy(m->dEdgeLut16, edgeLut16.data(), edgeLut16.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->dStart, m->tables.start, 257 * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->dData, m->tables.data.data(), 8192, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->dKey, packedKey.data(), 2432 * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess)
        return setError(MLSGPU_ERR_HIP, "Marching: table upload failed: %s", hipGetErrorString(e));
    *out = m.release();
    return MLSGPU_OK;
}

MLSGPU_API void mlsgpu_hip_marching_destroy(mlsgpu_marching *m)
{
    if (!m)
        return;
    hipSetDevice(m->ctx->device);
    delete m;
}

/* The lattice weld's generateCells (src/marching.cpp:500-551) for the buckets of a batch, one launch and one read-back:
 * totals[k] = the sum of the row totals of (sub-)swathe sws[k] of ms[k]; a single bucket is a batch of one */
static int rowTotalsLanes(mlsgpu_marching *const *ms, const mlsgpu_swathe *sws, uint32_t count, U3 *totals)
{
    mlsgpu_marching *m0 = ms[0];
    const auto rt = packLanes<RowTotalsArgs>(count, [&](uint32_t k) {
        const mlsgpu_swathe &sw = sws[k];
        const uint32_t cw = sw.width - 1, ch = sw.height - 1;
        const uint64_t rows = cw > 0 ? (uint64_t) ch * (sw.zLast - sw.zFirst) : 0;
        return RowTotalsArgs{ms[k]->dRowCounts + (uint64_t) (sw.zFirst - ms[k]->codeZ0) * ch, rows, &ms[k]->dReadback->totals};
    });
    uint32_t *const gate = m0->dReadback->gate;
    const uint32_t seq = m0->box.reserve();
    LAUNCH(m0->ctx, "kernel.marching.genOccupied.time", rowTotalsKernel, dim3(count), dim3(1024), rt, count, gate, m0->box.dev, seq);
    PROPAGATE(m0->box.wait(m0->ctx->stream));                /* the reference's queue.finish(), :548 */
    std::memcpy(totals, m0->box.payload(), count * sizeof(U3));
    return MLSGPU_OK;
}

/* generateCells, src/marching.cpp:500-551: the totals of the (sub-)swathe.  Lattice weld: from the row totals that
 * computeCodes left.  Sort weld: classifies the cells and leaves the scanned tile sums in dTileSums3 for the compaction pass. */
int mlsgpu_marching::generateCells(const mlsgpu_swathe &sw, U3 *totals)
{
    if (direct)
    {
        mlsgpu_marching *self = this;
        return rowTotalsLanes(&self, &sw, 1, totals);
    }
    const CellRange R{sw.width - 1, sw.height - 1, sw.zFirst};
    const uint64_t n = (uint64_t) R.cw * R.ch * (sw.zLast - sw.zFirst);
    ClassifyIn in{codeView(sw), R, dCount};
    PROPAGATE((scanPhase1<U3, ClassifyIn>(ctx, "kernel.marching.genOccupied.time", in, n, U3{0, 0, 0},
                                          dTileSums3, &dReadback->totals)));
    int pend = -1;
    if (ctx->timing) pend = ctx->beginTiming(ctx->statId("kernel.marching.readback.time"));
    PROPAGATE(box.publish(ctx->stream, &dReadback->totals, 3));
    if (pend >= 0) ctx->endTiming(pend);
    PROPAGATE(box.wait(ctx->stream));                    /* the reference's queue.finish(), :548 */
    std::memcpy(totals, box.payload(), sizeof(U3));
    return MLSGPU_OK;
}

int mlsgpu_marching::sliceHistogram(const mlsgpu_swathe &sw)
{
    const uint32_t slices = sw.zLast - sw.zFirst;
    LAUNCH(ctx, "kernel.marching.genOccupied.time", sliceHistogramKernel, dim3(slices), dim3(64),
           (const U3 *) dRowCounts, sw.height - 1, sw.zFirst, codeZ0, dHistogram);
    HIP_CHECK(hipMemcpyAsync(hHistogram + sw.zFirst, dHistogram + sw.zFirst, (size_t) slices * 8,
                             hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MLSGPU_OK;
}

template<typename K>
int mlsgpu_marching::weld(uint32_t nv, uint32_t zMax)
{
    K *keysA = reinterpret_cast<K *>(dKeysA.get()), *keysB = reinterpret_cast<K *>(dKeysB.get());
    SortResult<K> sorted;
    PROPAGATE(radixSort<K>(ctx, "kernel.marching.sortVertices.time", keysA, dValsA, keysB, dValsB, nv, layout.bits(),
                           true, dHist, dTileSums, &sorted));
    UniqueIn<K> in{sorted.keys, nv};
    CompactVerticesOut<K> outF{sorted.keys, sorted.vals, dVertices, dWelded, dWeldedKeys, dIndexRemap,
                               &dReadback->firstExternal, layout, 2 * zMax, packedKeyOffset(), nv, transform};
    return exclusiveScan<uint32_t>(ctx, "kernel.marching.compactVertices.time", in, outF, nv, 0u, dTileSums,
                                   &dReadback->numWelded);
}

/* cellCodeKernel over the cells of one top-level swathe */
CellCodeArgs mlsgpu_marching::cellCodeArgs(const mlsgpu_swathe &sw)
{
    const uint32_t cw = sw.width - 1, ch = sw.height - 1;
    const uint32_t rows = cw > 0 ? ch * (sw.zLast - sw.zFirst) : 0u;
    codeZ0 = sw.zFirst;
    return CellCodeArgs{dCellCode, dRowCounts, view(sw), cw, ch, sw.zFirst, rows, (const uchar2 *) dCount};
}

/* ... for the buckets of a batch (one launch); a single bucket is a batch of one */
static int computeCodesLanes(mlsgpu_marching *const *ms, const mlsgpu_swathe *sws, uint32_t count)
{
    mlsgpu_ctx *ctx = ms[0]->ctx;
    const auto L = packLanes<CellCodeArgs>(count, [&](uint32_t k) { return ms[k]->cellCodeArgs(sws[k]); });
    if (mostOfLanes(count, [&](uint32_t k) { return L.a[k].numRows; }) > 0)
    {
        /* a wave per 2 x 2 group of rows: the grid covers the lane with the most groups */
        const uint32_t maxGroups = mostOfLanes(count, [&](uint32_t k) {
            const CellCodeArgs &A = L.a[k];
            return A.ch > 0 ? (A.ch + 1) / 2 * ((A.numRows / A.ch + 1) / 2) : 0u;
        });
        LAUNCH(ctx, "kernel.marching.genOccupied.time", cellCodeKernel, dim3(divUp(maxGroups, 4), count), dim3(256), L);
    }
    return MLSGPU_OK;
}

int mlsgpu_marching::computeCodes(const mlsgpu_swathe &sw)
{
    mlsgpu_marching *self = this;
    return computeCodesLanes(&self, &sw, 1);
}

/* shipOut, src/marching.cpp:553-625, sort-based: works on the unwelded buffers filled by generateElements */
int mlsgpu_marching::shipOutSorted(uint32_t zMax, mlsgpu_mesh *mesh)
{
    const uint32_t nv = offsets[0], ni = offsets[1];
    if (wideKeys)
        PROPAGATE(weld<uint64_t>(nv, zMax));
    else
        PROPAGATE(weld<uint32_t>(nv, zMax));
    if (ni > 0)
        LAUNCH(ctx, "kernel.marching.reindex.time", reindexKernel, dim3(divUp(ni, 256)), dim3(256),
               dIndices, (const uint32_t *) dIndexRemap, ni);
    HIP_CHECK(hipMemcpyAsync(&hReadback->numWelded, &dReadback->numWelded, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));        /* the reference's queue.finish(), :617 */
    mesh->numVertices = hReadback->numWelded;
    mesh->numInternalVertices = hReadback->firstExternal;
    return MLSGPU_OK;
}

/* ------------------------------------------------------------------ ship-out of the lattice weld
 *
 * shipOut without a sort: the lattice weld over cells z in [zTop, zMax) of the resident swathe -- for every bucket of a
 * batch with ONE set of launches (blockIdx.y = bucket) and one read-back of all the welded counts.  A bucket of the batch
 * is a LatticeLane; every stage below takes the lanes of the batch, and shipOutLatticeLanes calls them in order. */
struct LatticeLane
{
    mlsgpu_marching *m;
    mlsgpu_swathe sw;
    uint32_t zTop, zMax;
    uint32_t cells, sizes[2];       /* occupied cells, vertices and indices accounted by addSlices */
    LatticeDims D;
    Lattice L;
    CodeView C;
    const U3 *firstRow;             /* the counts of the first row of cells */
    mlsgpu_mesh mesh;               /* out: the welded sizes filled in by latticeWeldedCounts */
};

static LatticeLane latticeLane(mlsgpu_marching *m, const mlsgpu_swathe &sw, uint32_t zTop, uint32_t zMax)
{
    const LatticeDims D(sw.width, sw.height, zTop, zMax);
    const Lattice L{m->dLatWords, m->dLatRows, &m->dReadback->classTotals, D.nw, D.rowsPerLayer, D.topx, D.topy,
                    D.z2First, D.z2Last, D.cw, D.ch};
    return LatticeLane{m, sw, zTop, zMax, m->bufferedCells, {m->offsets[0], m->offsets[1]}, D, L, m->codeView(sw),
                       m->dRowCounts + (uint64_t) (zTop - m->codeZ0) * D.ch, m->meshOf(m->offsets[1])};
}

typedef ScanJob<U3, ArrayIn<U3>, ArrayIn<U3>, ArrayOut<U3> > RowJob;

/* an exclusive scan of per-row counts in every lane: job(k) says from where to where */
template<typename Job>
static int scanRowCounts(mlsgpu_ctx *ctx, const char *stat, uint32_t count, Job job)
{
    RowJob jobs[MAX_LANES];
    for (uint32_t k = 0; k < count; k++)
        jobs[k] = job(k);
    return exclusiveScanBatch<U3, ArrayIn<U3>, ArrayIn<U3>, ArrayOut<U3> >(ctx, stat, jobs, count);
}

/* existence masks: the words of every lattice row and the row's vertices per class */
static int latticeMasks(const LatticeLane *lanes, uint32_t count)
{
    mlsgpu_ctx *ctx = lanes[0].m->ctx;
    const auto A = packLanes<LatticeMaskArgs>(count, [&](uint32_t k) {
        const LatticeLane &l = lanes[k];
        return LatticeMaskArgs{l.L, l.C, (const U3 *) l.m->dRowCounts, l.zTop, l.zMax, l.sw.height, l.D.cornerRows};
    });
    const char *const env = getenv("MLSGPU_HIP_LATTICE_MASK_ROWS");       /* read per ship-out: tests flip it */
    const bool forced = env != nullptr && atoi(env) != 0;
    bool byRows = false;                /* one launch for the batch: a lane that needs the rows kernel decides for all */
    for (uint32_t k = 0; k < count; k++)
        byRows = byRows || maskByRows(lanes[k].D.nw, forced);
    const uint32_t groups = mostOfLanes(count, [&](uint32_t k) { return lanes[k].D.maskGroups(byRows); });
    if (byRows)
        LAUNCH(ctx, "kernel.marching.countUniqueVertices.time", latticeMaskKernel, dim3(groups, count), dim3(256), A,
               (const uint64_t *) lanes[0].m->dEdgeLut);
    else
        LAUNCH(ctx, "kernel.marching.countUniqueVertices.time", latticeMaskWordKernel, dim3(std::max(groups, 1u), count), dim3(256), A,
               (const uint16_t *) lanes[0].m->dEdgeLut16);
    return MLSGPU_OK;
}

/* per-class start of every lattice row (the class totals land in classTotals), then absolute prefixes in the words */
static int latticeRowStarts(const LatticeLane *lanes, uint32_t count)
{
    mlsgpu_ctx *ctx = lanes[0].m->ctx;
    PROPAGATE(scanRowCounts(ctx, "kernel.marching.scanUint.time", count, [&](uint32_t k) {
        mlsgpu_marching *m = lanes[k].m;
        return RowJob{ArrayIn<U3>{m->dLatRows}, ArrayIn<U3>{m->dLatRows}, ArrayOut<U3>{m->dLatRows}, lanes[k].D.numRows,
                      U3{0, 0, 0}, m->dTileSums3, &m->dReadback->classTotals, nullptr};
    }));
    auto numWords = [&](uint32_t k) { return lanes[k].D.numWords(); };
    const auto A = packLanes<LatticePatchArgs>(count, [&](uint32_t k) { return LatticePatchArgs{lanes[k].L, numWords(k)}; });
    LAUNCH(ctx, "kernel.marching.scanUint.time", latticePatchKernel, dim3(divUp(mostOfLanes(count, numWords), 256), count), dim3(256), A);
    return MLSGPU_OK;
}

/* positions and external keys of the welded vertices */
static int latticeVertices(const LatticeLane *lanes, uint32_t count)
{
    mlsgpu_ctx *ctx = lanes[0].m->ctx;
    auto numQuads = [&](uint32_t k) { return lanes[k].D.numQuads(); };
    const auto A = packLanes<LatticeVerticesArgs>(count, [&](uint32_t k) {
        mlsgpu_marching *m = lanes[k].m;
        return LatticeVerticesArgs{lanes[k].L, m->view(lanes[k].sw), m->dWelded, m->dWeldedKeys, m->keyOffset[0], m->keyOffset[1],
                                   m->keyOffset[2], m->packedKeyOffset(), m->transform, numQuads(k)};
    });
    const dim3 grid(divUp(mostOfLanes(count, numQuads), 4), count);
    uint32_t enabled = 0;
    for (uint32_t k = 0; k < count; k++)
        enabled += lanes[k].m->transform.enabled ? 1u : 0u;
    if (enabled == count)
        LAUNCH(ctx, "kernel.marching.compactVertices.time", latticeVerticesKernel<1>, grid, dim3(256), A);
    else if (enabled == 0)
        LAUNCH(ctx, "kernel.marching.compactVertices.time", latticeVerticesKernel<0>, grid, dim3(256), A);
    else
        LAUNCH(ctx, "kernel.marching.compactVertices.time", latticeVerticesKernel<2>, grid, dim3(256), A);
    return MLSGPU_OK;
}

/* first cell / index slot of every row of cells of the batch (their totals land in batchTotals) */
static int cellRowStarts(const LatticeLane *lanes, uint32_t count)
{
    return scanRowCounts(lanes[0].m->ctx, "kernel.marching.scanElements.time", count, [&](uint32_t k) {
        const LatticeLane &l = lanes[k];
        return RowJob{ArrayIn<U3>{l.firstRow}, ArrayIn<U3>{l.firstRow}, ArrayOut<U3>{l.m->dRowStarts}, l.D.cellRows,
                      U3{0, 0, 0}, l.m->dTileSums3, &l.m->dReadback->batchTotals, nullptr};
    });
}

/* the triangles of the lanes that take the cells route: the compacted cells, then a thread per cell */
static int latticeTrianglesByCells(const LatticeLane *const *lanes, uint32_t count)
{
    mlsgpu_ctx *ctx = lanes[0]->m->ctx;
    const auto A = packLanes<CompactRowCellsArgs>(count, [&](uint32_t j) {
        const LatticeLane &l = *lanes[j];
        return CompactRowCellsArgs{(const uint8_t *) l.m->dCellCode, l.D.cw, l.D.ch, l.m->codeZ0, l.zTop,
                                   (const U3 *) l.m->dRowStarts, (const uchar2 *) l.m->dCount, l.m->dCells, l.m->dViStart,
                                   l.D.cellRows};
    });
    const auto B = packLanes<LatticeTrianglesArgs>(count, [&](uint32_t j) {
        const LatticeLane &l = *lanes[j];
        return LatticeTrianglesArgs{l.L, l.m->devTables(), (const uint2 *) l.m->dCells, (const uint2 *) l.m->dViStart,
                                    l.m->dIndices, (const U3 *) &l.m->dReadback->batchTotals};
    });
    const uint32_t mostRows = mostOfLanes(count, [&](uint32_t j) { return lanes[j]->D.cellRows; });
    const uint32_t mostCells = mostOfLanes(count, [&](uint32_t j) { return lanes[j]->cells; });
    LAUNCH(ctx, "kernel.marching.scanElements.time", compactRowCellsKernel, dim3(divUp(mostRows, 4), count), dim3(256), A);
    LAUNCH(ctx, "kernel.marching.generateElements.time", latticeTrianglesKernel, dim3(divUp(mostCells, 256), count), dim3(256), B);
    return MLSGPU_OK;
}

/* ... and of those that take the rows route: a wave per row of cells */
static int latticeTrianglesByRows(const LatticeLane *const *lanes, uint32_t count)
{
    mlsgpu_ctx *ctx = lanes[0]->m->ctx;
    const auto A = packLanes<LatticeTrianglesRowArgs>(count, [&](uint32_t j) {
        const LatticeLane &l = *lanes[j];
        return LatticeTrianglesRowArgs{l.L, l.C, l.m->devTables(), l.firstRow, (const U3 *) l.m->dRowStarts, l.zTop,
                                       l.m->dIndices, l.D.cellRows, l.m->dReadback->idle};
    });
    const uint32_t most = mostOfLanes(count, [&](uint32_t j) { return lanes[j]->D.cellRows; });
    const uint32_t nwMax = mostOfLanes(count, [&](uint32_t j) { return lanes[j]->D.nw; });
    /* dynamic LDS: the nine lattice rows of each of the four waves' rows of cells */
    LAUNCH_LDS(ctx, "kernel.marching.generateElements.time", latticeTrianglesRowKernel, dim3(divUp(most, 4), count), dim3(256),
               4 * 9 * nwMax * 16, A);
    return MLSGPU_OK;
}

/* the index list: every lane with cells by the route trianglesByCells gives it, each route one launch set */
static int latticeTriangles(const LatticeLane *lanes, uint32_t count)
{
    const char *const env = getenv("MLSGPU_HIP_TRIANGLES_BY_CELLS");      /* read per ship-out: tests flip it */
    const int forced = env == nullptr ? -1 : (env[0] != '0' ? 1 : 0);
    const LatticeLane *byCells[MAX_LANES], *byRows[MAX_LANES];
    uint32_t nc = 0, nr = 0;
    for (uint32_t k = 0; k < count; k++)
    {
        const LatticeLane &l = lanes[k];
        if (l.D.cellRows == 0 || l.cells == 0)
            continue;
        if (trianglesByCells(l.D.nw, l.cells, l.D.cellRows, l.D.cw, forced)) byCells[nc++] = &l; else byRows[nr++] = &l;
    }
    if (nc > 0)
        PROPAGATE(latticeTrianglesByCells(byCells, nc));
    if (nr > 0)
        PROPAGATE(latticeTrianglesByRows(byRows, nr));
    return MLSGPU_OK;
}

/* the welded counts of every bucket, one publication (classTotals and batchTotals are adjacent): what the device counted
 * is what addSlices accounted for, and the sizes of the meshes */
static int latticeWeldedCounts(LatticeLane *lanes, uint32_t count)
{
    mlsgpu_ctx *ctx = lanes[0].m->ctx;
    HostMailbox &box = lanes[0].m->box;
    const void *srcs[MAX_LANES];
    for (uint32_t k = 0; k < count; k++)
        srcs[k] = &lanes[k].m->dReadback->classTotals;
    PROPAGATE(box.publishGather(ctx->stream, srcs, count, 6));
    PROPAGATE(box.wait(ctx->stream));
    for (uint32_t k = 0; k < count; k++)
    {
        LatticeLane &l = lanes[k];
        U3 both[2];
        std::memcpy(both, box.payload() + 6 * k, sizeof(both));
        const U3 ct = both[0], bt = both[1];
        if (bt.a != l.cells || bt.b != l.sizes[0] || bt.c != l.sizes[1])
            return setError(MLSGPU_ERR_INVALID, "lattice weld: batch accounting mismatch (%u/%u cells, %u/%u vertices, %u/%u indices)",
                            bt.a, l.cells, bt.b, l.sizes[0], bt.c, l.sizes[1]);
        l.mesh.numVertices = (uint64_t) ct.a + ct.b + ct.c;
        l.mesh.numInternalVertices = ct.a;
    }
    return MLSGPU_OK;
}

static int shipOutLatticeLanes(LatticeLane *lanes, uint32_t count)
{
    REQUIRE(count >= 1 && count <= MAX_LANES, MLSGPU_ERR_INVALID);
    for (uint32_t k = 0; k < count; k++)
        REQUIRE(lanes[k].D.fits(lanes[k].m->latRowsMax, lanes[k].m->latWords), MLSGPU_ERR_LENGTH);
    PROPAGATE(latticeMasks(lanes, count));
    PROPAGATE(latticeRowStarts(lanes, count));
    PROPAGATE(latticeVertices(lanes, count));
    PROPAGATE(cellRowStarts(lanes, count));
    PROPAGATE(latticeTriangles(lanes, count));
    return latticeWeldedCounts(lanes, count);
}

/* the tail of shipOut (src/marching.cpp:619-624): counters, then the output functor */
int mlsgpu_marching::shipOutDone(const mlsgpu_mesh &mesh)
{
    counters[1]++;
    counters[4] += offsets[0];
    counters[5] += offsets[1];
    counters[6] += mesh.numVertices;
    counters[7] += mesh.numVertices - mesh.numInternalVertices;
    bufferedCells = 0;
    offsets[0] = offsets[1] = 0;
    if (output != nullptr)
    {
        const int rc = output(outputUser, outputIndex, ctx->stream, &mesh);
        if (rc != 0)
            return setError(MLSGPU_ERR_CALLBACK, "output functor failed with %d", rc);
    }
    return MLSGPU_OK;
}

/* shipOut, src/marching.cpp:553-625: what is buffered, cells z in [zTop, zMax) */
int mlsgpu_marching::shipOut(const mlsgpu_swathe &sw, uint32_t zMax)
{
    if (direct)
    {
        LatticeLane lane = latticeLane(this, sw, zTop, zMax);
        PROPAGATE(shipOutLatticeLanes(&lane, 1));
        return shipOutDone(lane.mesh);
    }
    mlsgpu_mesh mesh = meshOf(offsets[1]);
    PROPAGATE(shipOutSorted(zMax, &mesh));
    return shipOutDone(mesh);
}

/* addSlices, src/marching.cpp:627-743; `totals` are generateCells' of the (sub-)swathe */
int mlsgpu_marching::addSlices(const mlsgpu_swathe &swathe, const U3 &totals)
{
    const uint32_t compacted = totals.a;
    if (compacted > 0)
    {
        uint32_t counts[2] = {totals.b, totals.c};
        if (overflows(totals))
        {
            counters[0]++;
            ctx->addValue("marching.overflow", 1.0);                /* overflowStat, src/marching.cpp:655 */
            /* Swathe is too big on its own: split it into maximal runs of slices using the
             * per-slice histogram and recurse (:652-701). */
            PROPAGATE(sliceHistogram(swathe));
            std::vector<SliceCounts> hist;         /* a copy: the recursion may fill hHistogram again */
            for (uint32_t z = swathe.zFirst; z < swathe.zLast; z++)
                hist.push_back(SliceCounts{hHistogram[z].x, hHistogram[z].y});
            uint32_t subFirst = swathe.zFirst;
            while (subFirst < swathe.zLast)
            {
                const uint32_t subLast = swathe.zFirst + sliceRun(hist.data(), subFirst - swathe.zFirst, swathe.zLast - swathe.zFirst,
                                                                  offsets, vertexSpace, indexSpace);
                if (subLast <= subFirst)
                    return setError(MLSGPU_ERR_LENGTH, "Marching: a single slice exceeds the mesh memory");
                mlsgpu_swathe sub = swathe;
                sub.zFirst = subFirst;
                sub.zLast = subLast;
                U3 subTotals;
                PROPAGATE(generateCells(sub, &subTotals));
                PROPAGATE(addSlices(sub, subTotals));
                subFirst = subLast;
            }
        }
        else
        {
            if ((uint64_t) offsets[0] + counts[0] > vertexSpace || (uint64_t) offsets[1] + counts[1] > indexSpace)
            {
                /* fits, but only after flushing what is buffered (:705-719) */
                PROPAGATE(shipOut(swathe, swathe.zFirst));
                zTop = swathe.zFirst;
            }
            if (direct)
            {
                /* lattice weld: nothing to generate now -- the field stays resident, the ship-out works from it */
                bufferedCells += compacted;
            }
            else
            {
                /* scanElements + generateElements (:721-731): compaction pass, then one thread per cell */
                const uint32_t top[3] = {2 * (swathe.width - 1), 2 * (swathe.height - 1), 2 * zTop};
                const CellRange R{swathe.width - 1, swathe.height - 1, swathe.zFirst};
                const uint64_t n = (uint64_t) R.cw * R.ch * (swathe.zLast - swathe.zFirst);
                ClassifyIn in{codeView(swathe), R, dCount};
                CompactCellsOut outF{R, dCells, dViStart, offsets[0], offsets[1]};
                PROPAGATE((scanPhase2<U3, ClassifyIn, CompactCellsOut>(ctx, "kernel.marching.scanElements.time", in, outF, n,
                                                                       (const U3 *) dTileSums3)));
                const dim3 grid(divUp(compacted, 256)), block(256);
                if (wideKeys)
                    LAUNCH(ctx, "kernel.marching.generateElements.time", (generateElementsKernel<uint64_t>), grid, block,
                           dVertices, dKeysA.get(), dIndices, (const uint2 *) dViStart, (const uint2 *) dCells,
                           view(swathe), devTables(), keyOffset[0], keyOffset[1], keyOffset[2], top[0], top[1], top[2],
                           layout, compacted);
                else
                    LAUNCH(ctx, "kernel.marching.generateElements.time", (generateElementsKernel<uint32_t>), grid, block,
                           dVertices, reinterpret_cast<uint32_t *>(dKeysA.get()), dIndices, (const uint2 *) dViStart, (const uint2 *) dCells,
                           view(swathe), devTables(), keyOffset[0], keyOffset[1], keyOffset[2], top[0], top[1], top[2],
                           layout, compacted);
            }
            offsets[0] += counts[0];
            offsets[1] += counts[1];
            counters[3] += compacted;
        }
    }
    counters[2] += compacted > 0;
    ctx->addValue("marching.slices.nonempty", compacted > 0 ? 1.0 : 0.0);      /* nonemptyStat, src/marching.cpp:739 */
    return MLSGPU_OK;
}

/* the end of Marching::generate (src/marching.cpp:815-822): what is still buffered goes out, up to the swathe's last slice */
int mlsgpu_marching::endGenerate(const mlsgpu_swathe &sw)
{
    if (offsets[0] > 0)
        PROPAGATE(shipOut(sw, sw.zLast));
    ctx->addValue("marching.shipouts", (double) (counters[1] - shipOutsBefore));        /* shipoutsStat, src/marching.cpp:822 */
    return MLSGPU_OK;
}

/* the argument checks and per-call state of Marching::generate (src/marching.cpp:745-786) for bucket `index` of a call */
static int beginGenerate(mlsgpu_marching *m, const mlsgpu_generator *generator, mlsgpu_batch_output_fn output, void *outputUser,
                         uint32_t index, const uint32_t size[3], const uint32_t keyOffset[3], mlsgpu_swathe *swathe)
{
    REQUIRE(m != nullptr && generator != nullptr && generator->enqueue != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(size != nullptr && keyOffset != nullptr, MLSGPU_ERR_INVALID);
    swathe->width = size[0];
    swathe->height = size[1];
    swathe->zStride = m->zStride;
    const uint32_t depth = size[2];
    REQUIRE(1u <= swathe->width && swathe->width <= m->maxWidth, MLSGPU_ERR_LENGTH);
    REQUIRE(1u <= swathe->height && swathe->height <= m->maxHeight, MLSGPU_ERR_LENGTH);
    REQUIRE(1u <= depth && depth <= m->maxDepth, MLSGPU_ERR_LENGTH);
    /* global coordinates must fit the 20.1 key fields (MAX_GLOBAL_DIMENSION, src/marching.h:145-150) */
    for (int i = 0; i < 3; i++)
        REQUIRE((uint64_t) keyOffset[i] + size[i] <= (1u << 20) - 1, MLSGPU_ERR_LENGTH);
    m->output = output;
    m->outputUser = outputUser;
    m->outputIndex = index;
    for (int i = 0; i < 3; i++)
        m->keyOffset[i] = keyOffset[i];
    const KeyBits bits = keyLayout(size);
    m->layout = KeyLayout{bits.bx, bits.by, bits.bz};
    m->wideKeys = bits.wideKeys();
    const char *const force = getenv("MLSGPU_HIP_WELD");
    const WeldRoute route = weldRoute(depth, m->maxSwathe, m->legacyBuffers, force != nullptr && std::strcmp(force, "sort") == 0);
    if (route == WELD_NONE)
        return setError(MLSGPU_ERR_LENGTH, "Marching: depth %u needs several swathes but was created for one", depth);
    m->direct = route == WELD_LATTICE;
    m->bufferedCells = 0;
    m->offsets[0] = m->offsets[1] = 0;
    m->zTop = 0;
    m->shipOutsBefore = m->counters[1];
    return MLSGPU_OK;
}

static int callGenerator(const mlsgpu_generator *generator, mlsgpu_marching *m, const mlsgpu_swathe *swathe)
{
    const int rc = generator->enqueue(generator->user, m->ctx->stream, m->dField, m->imageWidth, swathe);
    if (rc != 0)
        return rc > 0 && rc <= MLSGPU_ERR_CALLBACK ? rc : setError(MLSGPU_ERR_CALLBACK, "generator failed with %d", rc);
    return MLSGPU_OK;
}

/* The swathe loop of Marching::generate (src/marching.cpp:787-824) for one bucket after beginGenerate: what a bucket of
 * several swathes, or one that takes the sort weld, goes through */
static int generateSwathes(mlsgpu_marching *m, const mlsgpu_generator *generator, mlsgpu_swathe swathe, uint32_t depth)
{
    for (uint32_t z = 0; z < depth; z += m->maxSwathe)
    {
        swathe.zFirst = z;
        swathe.zLast = std::min(depth, z + m->maxSwathe) - 1;
        swathe.zBias = (1 - (int32_t) z) * (int32_t) swathe.zStride;
        if (z != 0)
            PROPAGATE(mlsgpu_hip_marching_copy_slice(m, m->dField, m->imageWidth, m->maxSwathe, 0,
                                                     swathe.width, swathe.height, swathe.zStride));
        PROPAGATE(callGenerator(generator, m, &swathe));
        if (z > 0)
            swathe.zFirst--;
        PROPAGATE(m->computeCodes(swathe));
        U3 totals;
        PROPAGATE(m->generateCells(swathe, &totals));
        PROPAGATE(m->addSlices(swathe, totals));
    }
    return m->endGenerate(swathe);
}

extern "C" mlsgpu_mls *mlsgpu_hip_mls_of_generator(const mlsgpu_generator *gen);

/*
 * Marching::generate (src/marching.cpp:745-824) for the buckets of a batch (the SubItems of one WorkItem, which the
 * reference's worker walks one by one, src/workers.cpp:232-286); one bucket is a batch of one.  Every bucket has its own
 * Marching object (own field, lattice and mesh arena).  Meshes are handed to `output` bucket by bucket, in order.
 *
 * When every bucket takes the lattice weld (one swathe spans it) the batch runs in lock-step: every kernel launched once
 * with a bucket dimension, the swathe totals and the welded counts of all buckets read back together -- three host decisions
 * per BATCH.  Per bucket the results do not depend on its neighbours: the same kernels run on the same data, only the launch
 * is shared.  A bucket whose swathe overflows the mesh memory is split and shipped by addSlices when its turn comes (the
 * reference's slice splitting).  Otherwise -- a bucket needs several swathes, or MLSGPU_HIP_WELD=sort -- the buckets go
 * through generateSwathes one at a time.
 */
MLSGPU_API int mlsgpu_hip_marching_generate_batch(mlsgpu_marching *const *ms, const mlsgpu_generator *generators, uint32_t count,
                                                  mlsgpu_batch_output_fn output, void *outputUser,
                                                  const uint32_t *sizes, const uint32_t *keyOffsets)
{
    REQUIRE(ms != nullptr && generators != nullptr && sizes != nullptr && keyOffsets != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(count >= 1 && count <= MLSGPU_MAX_BATCH, MLSGPU_ERR_LENGTH);
    mlsgpu_swathe sws[MAX_LANES];
    for (uint32_t k = 0; k < count; k++)
    {
        REQUIRE(ms[k] != nullptr && ms[k]->ctx == ms[0]->ctx, MLSGPU_ERR_INVALID);
        for (uint32_t j = 0; j < k; j++)
            REQUIRE(ms[j] != ms[k], MLSGPU_ERR_INVALID);
    }
    mlsgpu_ctx *ctx = ms[0]->ctx;
    bool lockStep = true;
    for (uint32_t k = 0; k < count; k++)
    {
        PROPAGATE(beginGenerate(ms[k], &generators[k], output, outputUser, k, sizes + 3 * k, keyOffsets + 3 * k, &sws[k]));
        lockStep = lockStep && ms[k]->direct;
    }
    HIP_CHECK(hipSetDevice(ctx->device));
    if (!lockStep)
    {
        for (uint32_t k = 0; k < count; k++)
            PROPAGATE(generateSwathes(ms[k], &generators[k], sws[k], sizes[3 * k + 2]));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MLSGPU_OK;
    }
    /* every bucket is one swathe: slices [0, depth - 1], stored from row block 1 (src/marching.cpp:787-802) */
    mlsgpu_mls *functors[MAX_LANES];
    float *fields[MAX_LANES];
    uint64_t pitches[MAX_LANES];
    bool allMls = true;
    for (uint32_t k = 0; k < count; k++)
    {
        sws[k].zFirst = 0;
        sws[k].zLast = sizes[3 * k + 2] - 1;
        sws[k].zBias = (int32_t) sws[k].zStride;
        functors[k] = mlsgpu_hip_mls_of_generator(&generators[k]);
        allMls = allMls && functors[k] != nullptr;
        fields[k] = ms[k]->dField;
        pitches[k] = ms[k]->imageWidth;
    }
    if (allMls)
    {
        /* MlsFunctors: processCorners of the whole batch is one launch */
        const int rc = mlsgpu_hip_mls_enqueue_batch(functors, fields, pitches, nullptr, sws, count);
        if (rc != MLSGPU_OK)
            return rc;
    }
    else
        for (uint32_t k = 0; k < count; k++)
            PROPAGATE(callGenerator(&generators[k], ms[k], &sws[k]));
    PROPAGATE(computeCodesLanes(ms, sws, count));
    U3 totals[MAX_LANES];
    PROPAGATE(rowTotalsLanes(ms, sws, count, totals));
    /* The buckets whose swathe fits the mesh memory first: with nothing buffered addSlices only accounts for them on the
     * host, and their ship-outs at the end of the bucket share one set of launches. */
    LatticeLane ship[MAX_LANES];
    uint32_t numShip = 0;
    for (uint32_t k = 0; k < count; k++)
    {
        mlsgpu_marching *m = ms[k];
        if (m->overflows(totals[k]))
            continue;
        PROPAGATE(m->addSlices(sws[k], totals[k]));
        if (m->offsets[0] > 0)
            ship[numShip++] = latticeLane(m, sws[k], 0u, sws[k].zLast);
    }
    if (numShip > 0)
        PROPAGATE(shipOutLatticeLanes(ship, numShip));
    /* results bucket by bucket, in order; a bucket that has to be split is split and shipped here */
    for (uint32_t k = 0, next = 0; k < count; k++)
    {
        mlsgpu_marching *m = ms[k];
        if (next < numShip && ship[next].m == m)
            PROPAGATE(m->shipOutDone(ship[next++].mesh));
        else if (m->overflows(totals[k]))
            PROPAGATE(m->addSlices(sws[k], totals[k]));
        PROPAGATE(m->endGenerate(sws[k]));
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MLSGPU_OK;
}

/* Marching::generate, src/marching.cpp:745-824: a batch of one bucket */
namespace
{
struct SingleOutput
{
    mlsgpu_output_fn fn;
    void *user;
};
int singleOutput(void *user, uint32_t, void *stream, const mlsgpu_mesh *mesh)
{
    const SingleOutput *s = static_cast<const SingleOutput *>(user);
    return s->fn != nullptr ? s->fn(s->user, stream, mesh) : 0;
}
} // namespace

MLSGPU_API int mlsgpu_hip_marching_generate(mlsgpu_marching *m, const mlsgpu_generator *generator,
                                            mlsgpu_output_fn output, void *outputUser,
                                            const uint32_t size[3], const uint32_t keyOffset[3])
{
    SingleOutput single{output, outputUser};
    return mlsgpu_hip_marching_generate_batch(&m, generator, 1, singleOutput, &single, size, keyOffset);
}

MLSGPU_API int mlsgpu_hip_marching_set_vertex_transform(mlsgpu_marching *m, int enabled, float scale,
                                                        float bx, float by, float bz)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    m->transform = VertexTransform{scale, bx, by, bz, enabled ? 1 : 0};
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_marching_counters(const mlsgpu_marching *m, uint64_t out[8])
{
    REQUIRE(m != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    std::memcpy(out, m->counters, sizeof(m->counters));
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_marching_tables(const mlsgpu_marching *m, uint8_t *count, uint16_t *start, uint8_t *data, uint32_t *key)
{
    REQUIRE(m != nullptr, MLSGPU_ERR_INVALID);
    /* read back from the DEVICE copies so that the test sees what the kernels see */
    HIP_CHECK(hipSetDevice(m->ctx->device));
    HIP_CHECK(hipMemcpy(count, m->dCount, 512, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(start, m->dStart, 257 * 4, hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(data, m->dData, 8192, hipMemcpyDeviceToHost));
    std::vector<uint32_t> packed(2432);
    HIP_CHECK(hipMemcpy(packed.data(), m->dKey, 2432 * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < 2432; i++)
    {
        key[3 * i] = packed[i] & 0xFF;
        key[3 * i + 1] = (packed[i] >> 8) & 0xFF;
        key[3 * i + 2] = packed[i] >> 16;
    }
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_marching_copy_slice(mlsgpu_marching *m, float *dField, uint64_t pitch, uint32_t src, uint32_t trg,
                                              uint32_t width, uint32_t height, uint32_t zStride)
{
    REQUIRE(m != nullptr && dField != nullptr, MLSGPU_ERR_INVALID);
    if (width == 0 || height == 0)
        return MLSGPU_OK;
    LAUNCH(m->ctx, "kernel.marching.copySlice.time", copySliceKernel, dim3(divUp((uint64_t) width * height, 256)), dim3(256),
           dField, pitch, src * zStride, trg * zStride, width, height);
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_compact_vertices(mlsgpu_ctx *ctx, float *dOutVertices, uint64_t *dOutKeys, uint32_t *dIndexRemap,
                                           uint32_t *dFirstExternal, const uint32_t *dVertexUnique,
                                           const float *dInVertices4, const uint64_t *dInKeys,
                                           uint64_t minExternalKey, uint64_t keyOffset, uint64_t n)
{
    REQUIRE(ctx != nullptr, MLSGPU_ERR_INVALID);
    if (n == 0)
        return MLSGPU_OK;
    HIP_CHECK(hipSetDevice(ctx->device));
    LAUNCH(ctx, "kernel.marching.compactVertices.time", compactVerticesRefKernel, dim3(divUp(n, 64)), dim3(64),
           dOutVertices, dOutKeys, dIndexRemap, dFirstExternal, dVertexUnique,
           reinterpret_cast<const float4 *>(dInVertices4), dInKeys, minExternalKey, keyOffset, n);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_test_compute_key(mlsgpu_ctx *ctx, const uint32_t c[3], const uint32_t top[3], uint64_t *out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    HIP_CHECK(hipSetDevice(ctx->device));
    DeviceArray<uint64_t> d;
    PROPAGATE(d.alloc(1));
    hipLaunchKernelGGL(computeKeyTestKernel, dim3(1), dim3(1), 0, ctx->stream, c[0], c[1], c[2], top[0], top[1], top[2], d.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, d, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MLSGPU_OK;
}

/* ------------------------------------------------------------------ mesh plumbing */

MLSGPU_API uint64_t mlsgpu_hip_mesh_host_bytes(const mlsgpu_mesh *mesh)
{
    /* MeshSizes::getHostBytes, src/mesh.h:75-80 */
    return 12 * mesh->numVertices + 12 * mesh->numTriangles + 8 * (mesh->numVertices - mesh->numInternalVertices);
}

MLSGPU_API int mlsgpu_hip_mesh_read(mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh, void *hostBlob, int async)
{
    REQUIRE(ctx != nullptr && mesh != nullptr && hostBlob != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(mesh->numInternalVertices <= mesh->numVertices, MLSGPU_ERR_INVALID);             /* src/mesh.cpp:69 */
    REQUIRE(reinterpret_cast<uintptr_t>(hostBlob) % 8 == 0, MLSGPU_ERR_INVALID);             /* src/mesh.cpp:55 */
    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t numExt = mesh->numVertices - mesh->numInternalVertices;
    /* HostKeyMesh layout, src/mesh.cpp:51-60 */
    uint64_t *hKeys = static_cast<uint64_t *>(hostBlob);
    float *hVerts = reinterpret_cast<float *>(hKeys + numExt);
    uint32_t *hTris = reinterpret_cast<uint32_t *>(hVerts + 3 * mesh->numVertices);
    int pend = -1;
    if (ctx->timing) pend = ctx->beginTiming(ctx->statId("device.read"));
    if (mesh->numTriangles)
        HIP_CHECK(hipMemcpyAsync(hTris, mesh->dTriangles, mesh->numTriangles * 12, hipMemcpyDeviceToHost, ctx->stream));
    if (numExt)
        HIP_CHECK(hipMemcpyAsync(hKeys, mesh->dVertexKeys + mesh->numInternalVertices, numExt * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (mesh->numVertices)
        HIP_CHECK(hipMemcpyAsync(hVerts, mesh->dVertices, mesh->numVertices * 12, hipMemcpyDeviceToHost, ctx->stream));
    if (pend >= 0) ctx->endTiming(pend);
    if (!async)
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MLSGPU_OK;
}

/* Measurement aid: sum over the 32-bit words w[i] of an array of w[i] * (2 i + 1), modulo 2^64 -- sensitive to
 * values and to their order; partial sums per wave, one atomic per wave. */
namespace
{
__global__ __launch_bounds__(256) void checksumKernel(const uint32_t *words, uint64_t n, unsigned long long *out)
{
    unsigned long long acc = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        acc += (unsigned long long) words[i] * (2 * i + 1);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
        acc += __shfl_xor(acc, d, 64);
    if (laneId() == 0 && acc != 0)
        atomicAdd(out, acc);
}
} // namespace

MLSGPU_API int mlsgpu_hip_mesh_checksum(mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh, uint64_t out[3])
{
    REQUIRE(ctx != nullptr && mesh != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(mesh->numInternalVertices <= mesh->numVertices, MLSGPU_ERR_INVALID);
    HIP_CHECK(hipSetDevice(ctx->device));
    auto it = ctx->scratchCache.find("mesh.checksum");
    if (it == ctx->scratchCache.end())
    {
        void *d = nullptr;
        HIP_CHECK(hipMalloc(&d, 24));
        it = ctx->scratchCache.emplace("mesh.checksum", std::shared_ptr<void>(d, [](void *p) { hipFree(p); })).first;
    }
    unsigned long long *d = static_cast<unsigned long long *>(it->second.get());
    HIP_CHECK(hipMemsetAsync(d, 0, 24, ctx->stream));
    const uint64_t numExt = mesh->numVertices - mesh->numInternalVertices;
    const struct { const void *p; uint64_t words; } parts[3] = {
        {mesh->dVertices, 3 * mesh->numVertices}, {mesh->dTriangles, 3 * mesh->numTriangles},
        {mesh->dVertexKeys + mesh->numInternalVertices, 2 * numExt}};
    for (int k = 0; k < 3; k++)
        if (parts[k].words > 0)
            hipLaunchKernelGGL(checksumKernel, dim3((uint32_t) std::min<uint64_t>(divUp(parts[k].words, 256), 4096)), dim3(256), 0,
                               ctx->stream, static_cast<const uint32_t *>(parts[k].p), parts[k].words, d + k);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, d, 24, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_scale_bias(mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh, float scale, float bx, float by, float bz)
{
    REQUIRE(ctx != nullptr && mesh != nullptr, MLSGPU_ERR_INVALID);
    if (mesh->numVertices == 0)
        return MLSGPU_OK;           /* empty mesh is legal, test/test_mesh_filter.cpp:340-361 */
    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t n = mesh->numVertices * 3;
    LAUNCH(ctx, "kernel.scaleBias.time", scaleBiasKernel, dim3(divUp(n, 256)), dim3(256), mesh->dVertices, n, scale, bx, by, bz);
    return MLSGPU_OK;
}
