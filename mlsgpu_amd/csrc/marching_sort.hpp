/*
 * Part of marching.hip (its only includer): the classification of cells, which both welds start from, and the sort weld.
 *
 * Classification (genOccupied, kernels/marching.cl:84-120): the field and code-byte views, cellCodeKernel (a byte per cell
 * and each row's totals), the swathe totals and the per-slice histogram made of the row totals.
 *
 * Sort weld (the reference's structure: generateElements + sortVertices + countUnique + compactVertices + reindex), for
 * buckets of several swathes:
 *  - occupied cells are compacted in cell-linear (z, y, x) order by a three-component scan (cells, vertices, indices)
 *    whose producer classifies the cell and whose consumer writes the cell and its output positions: deterministic, and
 *    no global atomics (the reference appends with atomic_inc, kernels/marching.cl:114);
 *  - welding sorts (compact key, vertex index) pairs on only the significant key bits (1 + bits(2W) + bits(2H) + bits(2D)
 *    instead of 64) and moves the 16-byte positions once, in the compaction pass, instead of through every sort pass;
 *  - count-unique, its scan, compactVertices and the index remap table are one scan launch set.
 * The two kernels at the end serve known-answer tests only.
 */
#ifndef MLSGPU_MARCHING_SORT_HPP
#define MLSGPU_MARCHING_SORT_HPP

#include "marching_tables.hpp"
#include "primitives.hpp"

namespace
{

struct FieldView
{
    const float *field;
    uint64_t pitch;
    uint32_t zStride;
    int32_t zBias;
    __device__ __forceinline__ float at(uint32_t x, uint32_t row) const { return field[(uint64_t) row * pitch + x]; }
};

/* cell range of one (sub-)swathe: cells (x, y, z) with z in [zFirst, zLast) in (z, y, x) linear order */
struct CellRange
{
    uint32_t cw, ch;         /* cells per row / rows per slice (width-1, height-1) */
    uint32_t zFirst;
    __device__ __forceinline__ void decode(uint64_t i64, uint32_t &x, uint32_t &y, uint32_t &z) const
    {
        const uint32_t i = (uint32_t) i64;      /* swathe cells < 2^32, checked at creation */
        x = i % cw;
        const uint32_t r = i / cw;
        y = r % ch;
        z = r / ch + zFirst;
    }
};

__device__ __forceinline__ void loadIso(const FieldView &F, uint32_t x, uint32_t y, uint32_t z, float iso[8])
{
    /* kernels/marching.cl:95-107 */
    const uint32_t y0 = y + F.zStride * z + (uint32_t) F.zBias;
    const uint32_t y1 = y0 + F.zStride;
    iso[0] = F.at(x, y0);     iso[1] = F.at(x + 1, y0);
    iso[2] = F.at(x, y0 + 1); iso[3] = F.at(x + 1, y0 + 1);
    iso[4] = F.at(x, y1);     iso[5] = F.at(x + 1, y1);
    iso[6] = F.at(x, y1 + 1); iso[7] = F.at(x + 1, y1 + 1);
}

/* makeCode / isValid, kernels/marching.cl:41-63 */
__device__ __forceinline__ uint32_t cellCode(const float iso[8], bool &valid)
{
    uint32_t code = 0;
    valid = true;
#pragma unroll
    for (int i = 0; i < 8; i++)
    {
        code |= (iso[i] >= 0.0f ? 1u : 0u) << i;
        valid = valid && isfinite(iso[i]);
    }
    return code;
}

/* genOccupied (kernels/marching.cl:84-120), step 1: one byte per cell of the swathe = the cell's cube code if
 * the cell is occupied (all 8 corners finite, code not 0 / 255), else 0.  Every later pass (counting,
 * compaction, per-slice histogram, lattice weld) reads this byte instead of 8 floats. */
struct CodeView
{
    const uint8_t *codes;
    uint32_t cw, ch;
    uint32_t z0;             /* cell slice stored first */
    __device__ __forceinline__ uint32_t at(uint32_t x, uint32_t y, uint32_t z) const
    {
        return codes[((uint64_t) (z - z0) * ch + y) * cw + x];
    }
};

/* Code bytes plus each row's (occupied, vertices, indices) totals.  One wave per 2 x 2 group of rows of cells -- rows (y, z),
 * (y + 1, z), (y, z + 1), (y + 1, z + 1) -- lane = cell x: the four rows need nine rows of corners between them, not
 * sixteen, and (the kernel is bound by latency times resident waves, as latticeVerticesKernel) a wave has four rows' worth
 * of independent work behind one round of loads.  The row totals feed the swathe totals, the per-slice histogram and, in the
 * lattice weld, each row's first cell / index slot -- a 256x smaller scan than one over cells. */
#ifndef CELLCODE_RUN
#define CELLCODE_RUN 64
#endif
/* (the lattice kernels -- mask, vertices, triangle rows -- were tried the same way: no change, they do not wait for those rows) */
struct CellCodeArgs
{
    uint8_t *codes;
    U3 *rowCounts;
    FieldView F;
    uint32_t cw, ch, zFirst, numRows;
    const uchar2 *countTable;
};

__global__ __launch_bounds__(256) void cellCodeKernel(Lanes<CellCodeArgs> lanes)
{
    const CellCodeArgs A = lanes.a[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t cw = A.cw, ch = A.ch, zFirst = A.zFirst;
    const uint32_t slices = ch > 0 ? A.numRows / ch : 0u;
    const uint32_t groupsY = (ch + 1) / 2, groupsZ = (slices + 1) / 2;
    /* a group shares a third of its corner rows with the group one slice pair up, groupsY groups on: runs of CELLCODE_RUN
     * workgroups (a few slice pairs) stay on one XCD, whose L2 then serves that third */
    const uint32_t wg = runOfWorkgroup<CELLCODE_RUN>(blockIdx.x, (groupsY * groupsZ + 3) / 4);
    const uint32_t group = __builtin_amdgcn_readfirstlane(wg * 4 + (threadIdx.x >> 6));
    if (group >= groupsY * groupsZ)
        return;
    uint8_t *const codes = A.codes;
    U3 *const rowCounts = A.rowCounts;
    const FieldView F = A.F;
    const uchar2 *const countTable = A.countTable;
    const uint32_t y0 = 2 * (group % groupsY), zs0 = 2 * (group / groupsY);     /* zs: slice within the swathe */
    const bool hasY = y0 + 1 < ch, hasZ = zs0 + 1 < slices;
    /* the corner rows (y0 + a, z0 + b), a, b = 0..2, clamped into the rows the group uses */
    uint32_t corner[3][3];
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
        for (int a = 0; a < 3; a++)
            corner[b][a] = (y0 + min((uint32_t) a, hasY ? 2u : 1u)) + F.zStride * (zs0 + zFirst + min((uint32_t) b, hasZ ? 2u : 1u))
                           + (uint32_t) F.zBias;
    U3 sum[2][2] = {{U3{0u, 0u, 0u}, U3{0u, 0u, 0u}}, {U3{0u, 0u, 0u}, U3{0u, 0u, 0u}}};
    /* 192 cells at a time: the corner values of the three chunks are requested before the first code byte is stored (a load
     * issued behind a store waits for that store: loads and stores retire in order) */
    constexpr int C = 3;
    for (uint32_t x0 = 0; x0 < cw; x0 += 64 * C)
    {
        /* corner x of the nine corner rows; corner x + 1 is the next lane's, and lane 63's is lane 0's of the next chunk (the
         * corner after the last chunk is one more load) */
        float v[C + 1][3][3];
#pragma unroll
        for (int c = 0; c <= C; c++)
        {
            const uint32_t xc = min(x0 + 64 * c + (c < C ? lane : 0u), cw);
#pragma unroll
            for (int b = 0; b < 3; b++)
#pragma unroll
                for (int a = 0; a < 3; a++)
                    v[c][b][a] = F.at(xc, corner[b][a]);
        }
#pragma unroll
        for (int c = 0; c < C; c++)
        {
            if (x0 + 64 * c >= cw)
                break;
            const uint32_t x = x0 + 64 * c + lane;
            float n[3][3];      /* the same corners at x + 1 */
#pragma unroll
            for (int b = 0; b < 3; b++)
#pragma unroll
                for (int a = 0; a < 3; a++)
                {
                    const uint32_t next = readLane(__float_as_uint(v[c + 1][b][a]), 0);
                    const uint32_t down = waveShiftDown1(__float_as_uint(v[c][b][a]));
                    n[b][a] = __uint_as_float(lane == 63 ? next : down);
                }
#pragma unroll
            for (int dz = 0; dz < 2; dz++)
            {
                if (dz == 1 && !hasZ)
                    break;
#pragma unroll
                for (int dy = 0; dy < 2; dy++)
                {
                    if (dy == 1 && !hasY)
                        break;
                    if (x < cw)
                    {
                        /* loadIso's order, kernels/marching.cl:95-107 */
                        const float iso[8] = {v[c][dz][dy], n[dz][dy], v[c][dz][dy + 1], n[dz][dy + 1],
                                              v[c][dz + 1][dy], n[dz + 1][dy], v[c][dz + 1][dy + 1], n[dz + 1][dy + 1]};
                        bool valid;
                        uint32_t code = cellCode(iso, valid);
                        if (!valid || code == 255)
                            code = 0;
                        codes[((uint64_t) (zs0 + dz) * ch + (y0 + dy)) * cw + x] = (uint8_t) code;
                        if (code != 0)
                        {
                            const uchar2 cnt = countTable[code];
                            sum[dz][dy].a += 1;
                            sum[dz][dy].b += cnt.x;
                            sum[dz][dy].c += cnt.y;
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int dz = 0; dz < 2; dz++)
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
        {
            if ((dz == 1 && !hasZ) || (dy == 1 && !hasY))
                continue;
            U3 t = sum[dz][dy];
            t.a = waveSum(t.a);
            t.b = waveSum(t.b);
            t.c = waveSum(t.c);
            if (lane == 0)
                rowCounts[(uint64_t) (zs0 + dz) * ch + (y0 + dy)] = t;
        }
}

/* ... step 2: the producer of the compaction scan */
struct ClassifyIn
{
    CodeView C;
    CellRange R;
    const uchar2 *countTable;
    __device__ __forceinline__ U3 operator()(uint64_t i) const
    {
        uint32_t x, y, z;
        R.decode(i, x, y, z);
        const uint32_t code = C.at(x, y, z);
        if (code != 0)
        {
            const uchar2 c = countTable[code];
            return U3{1u, c.x, c.y};
        }
        return U3{0u, 0u, 0u};
    }
};

/* ... and its consumer: the compacted cell list and each cell's first vertex / index slot
 * (occupied / viCount after scanElements in the reference, src/marching.cpp:721) */
struct CompactCellsOut
{
    CellRange R;
    uint2 *cells;        /* x | y<<16, z */
    uint2 *viStart;
    uint32_t vBase, iBase;
    __device__ __forceinline__ void operator()(uint64_t i, U3 excl, U3 val) const
    {
        if (val.a)
        {
            uint32_t x, y, z;
            R.decode(i, x, y, z);
            cells[excl.a] = make_uint2(x | (y << 16), z);
            viStart[excl.a] = make_uint2(excl.b + vBase, excl.c + iBase);
        }
    }
};

/* The swathe totals of every bucket of a batch -- the sum of its row totals -- and their way to the host in ONE launch: a
 * workgroup per bucket adds up the bucket's rows, the last one to finish (a counter that wraps by itself; with one bucket
 * the only one) writes all the totals and the sequence number into the mailbox.  rowTotalsLanes is its one caller. */
struct RowTotalsArgs
{
    const U3 *rowCounts;
    uint64_t rows;
    U3 *total;
};

__global__ __launch_bounds__(1024) void rowTotalsKernel(Lanes<RowTotalsArgs> lanes, uint32_t count, uint32_t *gate,
                                                        uint32_t *box, uint32_t seq)
{
    const RowTotalsArgs A = lanes.a[blockIdx.x];
    __shared__ U3 waveTotals[16];
    U3 sum{0u, 0u, 0u};
    for (uint64_t i = threadIdx.x; i < A.rows; i += 1024)
        sum = sum + A.rowCounts[i];
    const U3 incl = waveInclusiveScanT(sum);
    if ((threadIdx.x & 63) == 63)
        waveTotals[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    U3 total = waveTotals[0];
    for (int w = 1; w < 16; w++)
        total = total + waveTotals[w];
    storeAgent(A.total, total);
    __threadfence();
    if (atomicInc(gate, count - 1) != count - 1)
        return;
    __threadfence();
    for (uint32_t k = 0; k < count; k++)
    {
        const U3 t = loadAgent(lanes.a[k].total);
        __hip_atomic_store(box + 1 + 3 * k, t.a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(box + 2 + 3 * k, t.b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(box + 3 + 3 * k, t.c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __threadfence_system();
    __hip_atomic_store(box, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

/* per-slice (vertices, indices) histogram, only needed by the overflow path (src/marching.cpp:652-701):
 * one wave per slice sums that slice's row totals */
__global__ __launch_bounds__(64) void sliceHistogramKernel(const U3 *rowCounts, uint32_t ch, uint32_t zFirst, uint32_t z0,
                                                           uint2 *histogram)
{
    const uint32_t z = zFirst + blockIdx.x;
    uint32_t v = 0, idx = 0;
    for (uint32_t y = threadIdx.x; y < ch; y += 64)
    {
        const U3 c = rowCounts[(uint64_t) (z - z0) * ch + y];
        v += c.b;
        idx += c.c;
    }
    v = waveSum(v);
    idx = waveSum(idx);
    if (threadIdx.x == 0)
        histogram[z] = make_uint2(v, idx);
}

/* ScaleBiasFilter (kernels/scale_bias.cl:33-41) folded into vertex emission: v = fma(v, scale, bias).
 * Same operation on the same rounded value as the separate in-place pass, one HBM round trip less. */
struct VertexTransform
{
    float scale, bx, by, bz;
    int enabled;
};

/* Layout of the compact sort key: [ext][z2 : bz][y2 : by][x2 : bx], order-isomorphic to the
 * reference's 64-bit key (kernels/marching.cl:148-154) for coordinates that fit the field widths. */
struct KeyLayout
{
    uint32_t bx, by, bz;
    __host__ __device__ __forceinline__ uint32_t bits() const { return bx + by + bz + 1; }
};

/* interp, kernels/marching.cl:130-138 (explicit fma, no other contraction) */
__device__ __forceinline__ void interp(float iso0, float iso1, uint32_t gx, uint32_t gy, uint32_t gz,
                                       uint32_t c0, uint32_t c1, float &ox, float &oy, float &oz)
{
    const float inv = 1.0f / (iso0 - iso1);
    const float t = iso0 * inv;
    const uint32_t o0x = c0 & 1, o0y = (c0 >> 1) & 1, o0z = (c0 >> 2) & 1;
    const uint32_t o1x = c1 & 1, o1y = (c1 >> 1) & 1, o1z = (c1 >> 2) & 1;
    ox = fmaf(t, (float) (o1x - o0x), (float) (gx + o0x));
    oy = fmaf(t, (float) (o1y - o0y), (float) (gy + o0y));
    oz = fmaf(t, (float) (o1z - o0z), (float) (gz + o0z));
}

__constant__ unsigned char dEdgeIndices[NUM_EDGES][2] =
{
    {0, 1}, {0, 2}, {0, 3}, {1, 3}, {2, 3}, {0, 4}, {0, 5}, {1, 5}, {4, 5}, {0, 6},
    {2, 6}, {4, 6}, {0, 7}, {1, 7}, {2, 7}, {3, 7}, {4, 7}, {5, 7}, {6, 7}
};

/* generateElements, kernels/marching.cl:184-258.  One thread per occupied cell.  Only the vertices
 * the cell's code uses are interpolated (the reference computes all 19 into local memory first);
 * a vertex's value does not depend on which others are computed. */
template<typename K>
__global__ __launch_bounds__(256) void generateElementsKernel(float4 *vertices, K *sortKeys, uint32_t *indices,
                                                              const uint2 *viStart, const uint2 *cells,
                                                              FieldView F, DevTables T,
                                                              uint32_t gox, uint32_t goy, uint32_t goz,
                                                              uint32_t topx, uint32_t topy, uint32_t topz,
                                                              KeyLayout L, uint32_t numCells)
{
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= numCells)
        return;
    const uint2 cell = cells[gid];
    const uint32_t x = cell.x & 0xFFFFu, y = cell.x >> 16, z = cell.y;
    float iso[8];
    loadIso(F, x, y, z, iso);
    bool valid;
    const uint32_t code = cellCode(iso, valid);
    const uint2 vi = viStart[gid];
    const ushort2 st = T.start[code], en = T.start[code + 1];
    const uint32_t nv = en.x - st.x, ni = en.y - st.y;
    const uint32_t gx = x + gox, gy = y + goy, gz = z + goz;
    for (uint32_t i = 0; i < nv; i++)
    {
        const uint32_t e = T.data[st.x + i];
        const uint32_t c0 = dEdgeIndices[e][0], c1 = dEdgeIndices[e][1];
        float vx, vy, vz;
        interp(iso[c0], iso[c1], gx, gy, gz, c0, c1, vx, vy, vz);
        vertices[vi.x + i] = make_float4(vx, vy, vz, __uint_as_float(vi.x + i));
        /* computeKey(2 * cell + keyTable[..], top), kernels/marching.cl:148-154,252 */
        const uint32_t k = T.key[st.x + i];
        const uint32_t kx = 2 * x + (k & 0xFF), ky = 2 * y + ((k >> 8) & 0xFF), kz = 2 * z + (k >> 16);
        const bool ext = kx == 0 || ky == 0 || kx == topx || ky == topy || kz == topz;
        sortKeys[vi.x + i] = ((K) (ext ? 1u : 0u) << (L.bx + L.by + L.bz)) | ((K) kz << (L.bx + L.by)) | ((K) ky << L.bx) | (K) kx;
    }
    for (uint32_t i = 0; i < ni; i++)
        indices[vi.y + i] = vi.x + T.data[st.y + i];
}

/* countUniqueVertices (kernels/marching.cl:271-279): 1 for the LAST of each run of equal keys.
 * The reference appends a ULONG_MAX sentinel; here the last element is simply always a run end. */
template<typename K>
struct UniqueIn
{
    const K *keys;
    uint64_t n;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        return (i + 1 >= n || keys[i] != keys[i + 1]) ? 1u : 0u;
    }
};

/* compactVertices (kernels/marching.cl:295-326) as the consumer of that scan.  Positions are
 * gathered here through the sorted vertex index instead of having travelled through the sort. */
template<typename K>
struct CompactVerticesOut
{
    const K *keys;
    const uint32_t *order;       /* sorted original vertex indices */
    const float4 *inVertices;
    float *outVertices;
    uint64_t *outKeys;
    uint32_t *indexRemap;
    uint32_t *firstExternal;
    KeyLayout L;
    uint32_t zMax2;              /* 2 * zMax: keys with z >= this are external (src/marching.cpp:593) */
    uint64_t keyOffset;
    uint64_t n;
    VertexTransform X;

    __device__ __forceinline__ bool isExternal(K key) const
    {
        const uint32_t z2 = (uint32_t) ((key >> (L.bx + L.by)) & (((K) 1 << L.bz) - 1));
        return ((key >> (L.bx + L.by + L.bz)) & 1) != 0 || z2 >= zMax2;
    }

    __device__ __forceinline__ void operator()(uint64_t i, uint32_t u, uint32_t isLast) const
    {
        const K key = keys[i];
        const uint32_t orig = order[i];
        if (isLast)
        {
            float4 v = inVertices[orig];
            if (X.enabled)
            {
                v.x = fmaf(v.x, X.scale, X.bx);
                v.y = fmaf(v.y, X.scale, X.by);
                v.z = fmaf(v.z, X.scale, X.bz);
            }
            outVertices[3 * (uint64_t) u + 0] = v.x;
            outVertices[3 * (uint64_t) u + 1] = v.y;
            outVertices[3 * (uint64_t) u + 2] = v.z;
            const bool ext = isExternal(key);
            const bool nextExt = (i + 1 >= n) || isExternal(keys[i + 1]);   /* sentinel counts as external */
            if (ext)
            {
                const uint64_t x2 = (uint64_t) (key & (((K) 1 << L.bx) - 1));
                const uint64_t y2 = (uint64_t) ((key >> L.bx) & (((K) 1 << L.by) - 1));
                const uint64_t z2 = (uint64_t) ((key >> (L.bx + L.by)) & (((K) 1 << L.bz) - 1));
                outKeys[u] = ((z2 << (2 * KEY_AXIS_BITS)) | (y2 << KEY_AXIS_BITS) | x2) + keyOffset;
                if (u == 0)
                    *firstExternal = 0;
            }
            else if (nextExt)
                *firstExternal = u + 1;
        }
        indexRemap[orig] = u;
    }
};

/* reindex, kernels/marching.cl:334-340 */
__global__ __launch_bounds__(256) void reindexKernel(uint32_t *indices, const uint32_t *indexRemap, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        indices[i] = indexRemap[indices[i]];
}

/* the reference's compactVertices kernel verbatim in behaviour, for its known-answer test */
__global__ void compactVerticesRefKernel(float *outVertices, uint64_t *outKeys, uint32_t *indexRemap,
                                         uint32_t *firstExternal, const uint32_t *vertexUnique,
                                         const float4 *inVertices, const uint64_t *inKeys,
                                         uint64_t minExternalKey, uint64_t keyOffset, uint64_t n)
{
    const uint64_t gid = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n)
        return;
    const uint32_t u = vertexUnique[gid];
    const float4 v = inVertices[gid];
    const uint64_t key = inKeys[gid];
    const uint64_t nextKey = inKeys[gid + 1];
    const bool ext = key >= minExternalKey;
    if (key != nextKey)
    {
        outVertices[3 * (uint64_t) u + 0] = v.x;
        outVertices[3 * (uint64_t) u + 1] = v.y;
        outVertices[3 * (uint64_t) u + 2] = v.z;
        if (ext)
        {
            outKeys[u] = (key & (KEY_EXTERNAL_FLAG - 1)) + keyOffset;
            if (u == 0)
                *firstExternal = 0;
        }
        else if (nextKey >= minExternalKey)
            *firstExternal = u + 1;
    }
    indexRemap[__float_as_uint(v.w)] = u;
}

__global__ void computeKeyTestKernel(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t tx, uint32_t ty, uint32_t tz,
                                     uint64_t *out)
{
    /* computeKey, kernels/marching.cl:148-154 */
    uint64_t key = ((uint64_t) cz << (2 * KEY_AXIS_BITS)) | ((uint64_t) cy << KEY_AXIS_BITS) | (uint64_t) cx;
    if (cx == 0 || cy == 0 || cx == tx || cy == ty || cz == tz)
        key |= KEY_EXTERNAL_FLAG;
    *out = key;
}

} // namespace

#endif
