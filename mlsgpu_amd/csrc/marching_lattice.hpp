/*
 * Part of marching.hip (its only includer): the lattice weld, the weld of a bucket that one swathe spans.  Its kernels in
 * launch order: a mask kernel (latticeMaskWordKernel, or latticeMaskKernel for rows of more than 64 words), the scan of the
 * rows' counts (primitives.hpp), latticePatchKernel, latticeVerticesKernel, the scan of the rows of cells, then the
 * triangles by rows (latticeTrianglesRowKernel) or by cells (compactRowCellsKernel, latticeTrianglesKernel).  The host
 * side -- the geometry, the launch counts and the rules that choose between the kernels -- is marchingplan.hpp, the
 * launches themselves the ship-out stages of marching.hip.  The field and code-byte views and VertexTransform come from
 * marching_sort.hpp.
 *
 * Sort-free replacement for generateElements + sortVertices + countUnique + compactVertices + reindex,
 * used when the whole batch lies in the resident field (one swathe per bucket, the MI355X default).
 *
 * Every welded vertex sits on a grid edge whose endpoints have different signs, i.e. on one point of
 * the HALF LATTICE (x2, y2, z2) = 2*cell + keyTable offset -- exactly the fixed-point coordinates the
 * reference packs into its vertex key (kernels/marching.cl:148-154,252).  Sorting by key therefore
 * equals enumerating half-lattice points in (z2, y2, x2) order, and a welded vertex's index is its
 * rank in that order within its class:
 *     class 0  internal                        (first in the output)
 *     class 1  unflagged, z2 == 2*zMax         (external by "key >= minExternalKey", src/marching.cpp:593)
 *     class 2  flagged (x2 == 0, y2 == 0, x2 == top.x, y2 == top.y or z2 == top.z; marching.cl:151-152)
 * which is the order the reference's 64-bit sort produces (flag bit above z above y above x).
 * A vertex exists on an edge iff some OCCUPIED cell of the batch contains the edge and sees different
 * signs at its ends (every sign-changing edge of a cell is used by one of its tetrahedra, so this is
 * exactly the set of vertices the per-cell tables emit).
 *
 * Rows are (z2, y2); each row is a bit mask over x2 plus per-word prefix counts, so an index is
 * rowStart[class] + wordPrefix + popcount -- three small L2-resident reads instead of a global sort.
 */
#ifndef MLSGPU_MARCHING_LATTICE_HPP
#define MLSGPU_MARCHING_LATTICE_HPP

#include "marching_sort.hpp"

namespace
{

/* One 64-point word of a row, 16 bytes, everything a lookup needs in ONE load:
 *   mask    existence bits of the row's MAIN class (all points of a class-2 row; a class-0/1 row without its two
 *           class-2 columns x2 == 0 and x2 == top.x)
 *   prefix  output index of the first main-class vertex of this word (row-relative until latticePatchKernel
 *           adds the row's start)
 *   flag    class-0/1 rows: output index of the row's first class-2 vertex, bit 31 = a vertex exists at x2 == 0,
 *           bit 30 = one exists at x2 == top.x (latticeMaskKernel sets each bit in the word that holds the column;
 *           latticePatchKernel copies both into every word of the row and adds the index) */
struct LatWord
{
    uint64_t mask;
    uint32_t prefix;
    uint32_t flag;
};
#define LAT_FLAG_X0 0x80000000u
#define LAT_FLAG_TOP 0x40000000u
#define LAT_FLAG_INDEX 0x3FFFFFFFu

struct Lattice
{
    LatWord *words;          /* [rows][nw] */
    U3 *rowCounts;           /* [rows] vertices per class; exclusive-scanned in place into per-class row starts */
    const U3 *totals;        /* device: class totals after the scan */
    uint32_t nw;             /* 64-bit words per row */
    uint32_t rowsPerLayer;   /* 2H - 1 */
    uint32_t topx, topy;     /* 2(W-1), 2(H-1) */
    uint32_t z2First;        /* 2 * zTop: first layer, also top.z */
    uint32_t z2Last;         /* 2 * zMax: last layer */
    uint32_t cw, ch;         /* cells per row / rows of cells */

    __device__ __forceinline__ uint32_t rowClass(uint32_t y2, uint32_t z2) const
    {
        if (y2 == 0 || y2 == topy || z2 == z2First)
            return 2;
        return z2 == z2Last ? 1 : 0;
    }
    __device__ __forceinline__ bool rowFlagged(uint32_t y2, uint32_t z2) const { return rowClass(y2, z2) == 2; }
    /* bits of word w that belong to columns x2 == 0 and x2 == top.x (class 2 inside class 0/1 rows) */
    __device__ __forceinline__ uint64_t columnMask(uint32_t w) const
    {
        uint64_t m = w == 0 ? 1ull : 0ull;
        if (w == (topx >> 6))
            m |= 1ull << (topx & 63);
        return m;
    }
};

/* a finished row's vertices per class: `main` of its own class and `columns` of class 2 in its two columns */
__device__ __forceinline__ U3 latticeRowCount(uint32_t cls, uint32_t main, uint32_t columns)
{
    U3 cnt{0u, 0u, 0u};
    if (cls == 0) { cnt.a = main; cnt.c = columns; }
    else if (cls == 1) { cnt.b = main; cnt.c = columns; }
    else cnt.c = main;
    return cnt;
}

/* the output index of a class-0/1 row's class-2 vertex at x2 == 0 or (top) at x2 == top.x, from the row's flag word: the
 * one at top.x follows the one at 0 where that exists */
template<bool TOP>
__device__ __forceinline__ uint32_t columnVertex(uint32_t flag)
{
    if constexpr (TOP)
        return (flag & LAT_FLAG_INDEX) + (flag >> 31);
    else
        return flag & LAT_FLAG_INDEX;
}

/* where a cell's edge e has its lattice point: (2x + px, 2y + py, 2z + pz) of cell (x, y, z); q = the point's row among the
 * cell's nine, (2y + q % 3, 2z + q / 3) */
struct EdgePoint
{
    int a, b;            /* the edge's local corners */
    int px, py, pz, q;
};
constexpr EdgePoint edgePoint(int e)
{
    const int a = edgeIndices[e][0], b = edgeIndices[e][1];
    const int px = (a & 1) + (b & 1), py = ((a >> 1) & 1) + ((b >> 1) & 1), pz = ((a >> 2) & 1) + ((b >> 2) & 1);
    return EdgePoint{a, b, px, py, pz, py + 3 * pz};
}

/* does a cell with this code (0 = not occupied) see different signs at its local corners a and b? */
__device__ __forceinline__ uint32_t edgeBit(uint32_t code, uint32_t a, uint32_t b)
{
    return ((code >> a) ^ (code >> b)) & 1u;
}

/*
 * Existence masks.  One wave per row of CORNERS (fixed y, z), lane = corner x.  A corner owns the seven
 * edges towards +x, +y, +z, +xy, +xz, +yz, +xyz, i.e. the half-lattice points of four rows:
 *   (z2, y2) = (2z, 2y): +x at x2 = 2x+1          (2z, 2y+1): +y at 2x, +xy at 2x+1
 *              (2z+1, 2y): +z at 2x, +xz at 2x+1  (2z+1, 2y+1): +yz at 2x, +xyz at 2x+1
 * An edge carries a vertex iff one of the occupied cells containing it sees a sign change along it; those
 * cells are among the eight around the corner, whose code bytes are four loads per lane (cell x of the four
 * adjacent cell rows) plus a lane shift for cell x-1.  The seven bits of 64 corners become the rows' words
 * (even/odd x2 interleaved) through two lane permutations and one ballot per word.
 * edgeLut (dEdgeLut, which feeds this kernel only) is makeEdgeLut's table: per code byte, the lattice points a cell gives
 * a corner.
 *
 * This kernel and latticeMaskWordKernel must agree bit for bit (test_mask_kernels_agree) and write out, each for itself, the
 * test for an adjacent row of cells, the four lattice rows of a corner row (id, class, exists) and the split of a word
 * into main bits, column count and flag bits: shared functions for these changed the instructions of both kernels
 * (profiles/NOTES_marching_split.md).  Change the two together.
 */
struct LatticeMaskArgs
{
    Lattice L;
    CodeView C;
    const U3 *cellRowCounts;
    uint32_t zCellFirst, zCellLast, H, numCornerRows;
};

__global__ __launch_bounds__(256) void latticeMaskKernel(Lanes<LatticeMaskArgs> lanes, const uint64_t *edgeLut)
{
    __shared__ uint64_t sLut[256];
    sLut[threadIdx.x] = edgeLut[threadIdx.x];
    __syncthreads();
    const LatticeMaskArgs A = lanes.a[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t cr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cr >= A.numCornerRows)
        return;
    const Lattice L = A.L;            /* a copy: the fields live in scalar registers, not behind kernel-argument loads */
    const CodeView C = A.C;
    const U3 *const cellRowCounts = A.cellRowCounts;
    const uint32_t zCellFirst = A.zCellFirst, zCellLast = A.zCellLast, H = A.H;
    const uint32_t y = cr % H, z = cr / H + zCellFirst;
    const uint32_t W = L.cw + 1;
    /* adjacent cell rows (y - dy, z - dz); a row outside the batch contributes no occupied cell */
    bool rowOk[2][2];
    const uint8_t *rowPtr[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dz = 0; dz < 2; dz++)
        {
            const int cy = (int) y - dy, cz = (int) z - dz;
            rowOk[dy][dz] = cy >= 0 && cy < (int) L.ch && cz >= (int) zCellFirst && cz < (int) zCellLast;
            rowPtr[dy][dz] = C.codes + ((uint64_t) ((uint32_t) cz - C.z0) * C.ch + (uint32_t) cy) * C.cw;
        }
    uint32_t rowId[4], rowCls[4], running[4], nFlag[4];
    bool rowExists[4];
#pragma unroll
    for (int h = 0; h < 4; h++)
    {
        const uint32_t y2 = 2 * y + (h & 1), z2 = 2 * z + (h >> 1);
        rowExists[h] = y2 <= L.topy && z2 <= L.z2Last;
        rowId[h] = (z2 - L.z2First) * L.rowsPerLayer + y2;
        rowCls[h] = L.rowClass(y2, z2);
        running[h] = nFlag[h] = 0;
    }
    /* (the first code bytes are requested before the rows' totals are looked at: one latency, not two) */
    uint32_t next[2][2];
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dz = 0; dz < 2; dz++)
            next[dy][dz] = (rowOk[dy][dz] && lane < L.cw) ? rowPtr[dy][dz][lane] : 0u;
    /* Surface-like data leaves most of a bucket empty: if none of the adjacent cell rows holds an occupied cell (their
     * totals come from cellCodeKernel) the four rows are all zeros, written by 16-byte stores of the first lanes. */
    uint32_t occupied = 0;
#pragma unroll
    for (int dy = 0; dy < 2; dy++)
#pragma unroll
        for (int dz = 0; dz < 2; dz++)
            if (rowOk[dy][dz])
                occupied += cellRowCounts[(uint64_t) ((uint32_t) ((int) z - dz) - C.z0) * C.ch + (uint32_t) ((int) y - dy)].a;
    if (occupied == 0)
    {
#pragma unroll
        for (int h = 0; h < 4; h++)
        {
            if (!rowExists[h])
                continue;
            for (uint32_t w = lane; w < L.nw; w += 64)
                L.words[(uint64_t) rowId[h] * L.nw + w] = LatWord{0ull, 0u, 0u};
            if (lane == 0)
                L.rowCounts[rowId[h]] = U3{0u, 0u, 0u};
        }
        return;
    }
    uint32_t prevLeft = 0;
    for (uint32_t x0 = 0; x0 < W; x0 += 64)
    {
        /* What the cell at (x - ox, y - dy, z - dz) gives the corner's seven points depends on its code byte alone: a table
         * (makeEdgeLut) holds, per code, the bits of each of the four (dy, dz) as the corner's own cell (ox = 0, bytes 0-3)
         * and as the cell to its left (ox = 1, bytes 4-7).  The left cell of lane i is lane i - 1's own, so its bits come
         * with one lane shift; 64 corners further the carry is lane 63's. */
        uint32_t own = 0, left = 0;
#pragma unroll
        for (int dy = 0; dy < 2; dy++)
#pragma unroll
            for (int dz = 0; dz < 2; dz++)
            {
                const uint32_t c = next[dy][dz];
                const uint32_t xn = x0 + 64 + lane;
                next[dy][dz] = (rowOk[dy][dz] && xn < L.cw) ? rowPtr[dy][dz][xn] : 0u;
                const uint64_t v = sLut[c];
                const int r = dy | (dz << 1);
                own |= ((uint32_t) v >> (8 * r)) & 0xFFu;
                left |= ((uint32_t) (v >> 32) >> (8 * r)) & 0xFFu;
            }
        const uint32_t up = waveShiftUp1(left);
        /* bit 0 +x, 1 +xy, 2 +xz, 3 +xyz (odd x2 of rows h = 0..3), 5 +y, 6 +z, 7 +yz (even x2 of rows 1..3) */
        const uint32_t pk = own | (lane == 0 ? prevLeft : up);
        prevLeft = readLane(left, 63);
        /* Interleave (even x2 = 2x, odd x2 = 2x+1) by lane permutation instead of bit spreading: lane i of word
         * `half` takes corner 32*half + i/2 and its even (i even) or odd (i odd) point, so one ballot per row and
         * half IS the 64-bit word. */
        const uint32_t from[2] = {(uint32_t) __shfl(pk, lane >> 1, 64), (uint32_t) __shfl(pk, 32 + (lane >> 1), 64)};
        const uint32_t sel = (lane & 1) ? 0u : 4u;
#pragma unroll
        for (int h = 0; h < 4; h++)
        {
            if (!rowExists[h])
                continue;
#pragma unroll
            for (int half = 0; half < 2; half++)
            {
                const uint32_t w = (x0 >> 6) * 2 + half;
                if (w >= L.nw)
                    continue;
                const uint64_t bits = __ballot((from[half] >> (sel + h)) & 1u);
                const uint64_t cm = rowCls[h] == 2 ? 0ull : L.columnMask(w);
                const uint64_t col = bits & cm;
                const uint64_t topBit = w == (L.topx >> 6) ? 1ull << (L.topx & 63) : 0ull;
                const uint32_t colBits = ((w == 0 && (col & 1ull)) ? LAT_FLAG_X0 : 0u) | ((col & topBit) ? LAT_FLAG_TOP : 0u);
                if (lane == 0)
                    L.words[(uint64_t) rowId[h] * L.nw + w] = LatWord{bits & ~cm, running[h], colBits};
                running[h] += (uint32_t) __popcll(bits & ~cm);
                nFlag[h] += (uint32_t) __popcll(col);
            }
        }
    }
    if (lane == 0)
    {
#pragma unroll
        for (int h = 0; h < 4; h++)
            if (rowExists[h])
            {
                U3 cnt{0u, 0u, 0u};
                if (rowCls[h] == 0) { cnt.a = running[h]; cnt.c = nFlag[h]; }
                else if (rowCls[h] == 1) { cnt.b = running[h]; cnt.c = nFlag[h]; }
                else cnt.c = running[h];
                L.rowCounts[rowId[h]] = cnt;
            }
    }
}

/*
 * The same masks, one THREAD per 64-bit word (32 corners) instead of one wave per row of corners.  The wave-per-row kernel
 * above spends ~730 vector and ~460 scalar instructions per row of 171 corners -- seven ballots per 64 corners, each followed
 * by scalar mask arithmetic and a 16-byte store from one lane -- and is bound by issuing them (VALU 61 %, one scalar unit per
 * CU 58 % busy; profiles/r05b_sq_stage_kernels.csv): 0.95 ms per step for 0.35 GB.  Here a lane walks its word's 32 corners
 * with bit operations of its own: per corner four table lookups (what the cell (x, y - dy, z - dz) gives the corner as its
 * own cell, low byte, and as the cell to its left, high byte; bits 2h + 1 / 2h = the odd / even point of lattice row h),
 * three ORs and four two-bit inserts -- ~22 vector instructions per corner and LANE, i.e. a third of an instruction per
 * corner and wave.  The lanes of a row of corners (nw consecutive ones; 64 / nw rows per wave) exchange their popcounts for
 * the words' prefixes, and every lattice row leaves as one run of 16-byte stores.  Words, counts and flags are the ones
 * the wave-per-row kernel writes, bit for bit (MLSGPU_HIP_LATTICE_MASK_ROWS=1 selects it for A/B).
 * edgeLut16 (dEdgeLut16, which feeds this kernel only) is makeEdgeLut16's table: the same per (dy, dz).
 */
__global__ __launch_bounds__(256) void latticeMaskWordKernel(Lanes<LatticeMaskArgs> lanes, const uint16_t *edgeLut16)
{
    __shared__ uint16_t sLut[4][256];
    for (uint32_t i = threadIdx.x; i < 1024; i += 256)
        (&sLut[0][0])[i] = edgeLut16[i];
    __syncthreads();
    const LatticeMaskArgs A = lanes.a[blockIdx.y];
    const Lattice L = A.L;
    const CodeView C = A.C;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = L.nw, rowsPerWave = 64u / nw;
    const uint32_t sub = lane / nw, w = lane - sub * nw;
    const uint32_t cr = (blockIdx.x * 4 + (threadIdx.x >> 6)) * rowsPerWave + sub;
    const bool active = sub < rowsPerWave && cr < A.numCornerRows;
    const uint32_t H = A.H, zCellFirst = A.zCellFirst, zCellLast = A.zCellLast;
    const uint32_t crc = active ? cr : 0u;
    const uint32_t y = crc % H, z = crc / H + zCellFirst;
    const uint32_t cw = L.cw;
    const uint32_t x0 = 32u * w;                 /* the word's first corner */

    /* the word's 4 x 32 code bytes (cell x of the four adjacent rows of cells), and the byte before them; the bytes behind a
     * row's end are the next row's (or the buffer's pad) and are masked away */
    uint32_t keep[8];
    {
        const uint32_t have = x0 < cw ? min(cw - x0, 32u) : 0u;
#pragma unroll
        for (int j = 0; j < 8; j++)
        {
            const uint32_t n = have > 4u * j ? min(have - 4u * j, 4u) : 0u;      /* bytes of dword j that exist */
            keep[j] = n >= 4u ? 0xFFFFFFFFu : (1u << (8u * n)) - 1u;
        }
    }
    uint32_t cd[4][8], before[4];
    uint32_t occupied = 0;
#pragma unroll
    for (int r = 0; r < 4; r++)
    {
        const int dy = r & 1, dz = r >> 1;
        const int cy = (int) y - dy, cz = (int) z - dz;
        const bool ok = active && cy >= 0 && cy < (int) L.ch && cz >= (int) zCellFirst && cz < (int) zCellLast;
        const uint64_t rowIndex = ok ? (uint64_t) ((uint32_t) cz - C.z0) * C.ch + (uint32_t) cy : 0ull;
        const uint8_t *const rowBase = C.codes + rowIndex * C.cw;
        const uint8_t *p = rowBase + (x0 < cw ? x0 : 0u);
        if (ok)
            occupied += A.cellRowCounts[rowIndex].a;
        uint4 lo = make_uint4(0, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
        if (ok && x0 < cw)
        {
            __builtin_memcpy(&lo, p, 16);
            __builtin_memcpy(&hi, p + 16, 16);
        }
        cd[r][0] = lo.x & keep[0]; cd[r][1] = lo.y & keep[1]; cd[r][2] = lo.z & keep[2]; cd[r][3] = lo.w & keep[3];
        cd[r][4] = hi.x & keep[4]; cd[r][5] = hi.y & keep[5]; cd[r][6] = hi.z & keep[6]; cd[r][7] = hi.w & keep[7];
        before[r] = (ok && x0 > 0 && x0 - 1 < cw) ? (uint32_t) rowBase[x0 - 1] : 0u;     /* (a word may begin AT the row's end) */
    }

    /* the four lattice rows of the corner row: h = py | pz << 1 */
    uint64_t bits[4] = {0, 0, 0, 0};
    if (occupied != 0)
    {
        uint32_t lo32[4] = {0, 0, 0, 0}, hi32[4] = {0, 0, 0, 0};
        /* what the cell left of the word's first corner gives it */
        uint32_t leftPrev = ((uint32_t) sLut[0][before[0]] | sLut[1][before[1]] | sLut[2][before[2]] | sLut[3][before[3]]) >> 8;
#pragma unroll
        for (int i = 0; i < 32; i++)
        {
            const uint32_t e = (uint32_t) sLut[0][(cd[0][i >> 2] >> (8 * (i & 3))) & 0xFFu]
                | sLut[1][(cd[1][i >> 2] >> (8 * (i & 3))) & 0xFFu]
                | sLut[2][(cd[2][i >> 2] >> (8 * (i & 3))) & 0xFFu]
                | sLut[3][(cd[3][i >> 2] >> (8 * (i & 3))) & 0xFFu];
            const uint32_t pk = (e & 0xFFu) | leftPrev;
            leftPrev = e >> 8;
#pragma unroll
            for (int h = 0; h < 4; h++)
            {
                const uint32_t pair = (pk >> (2 * h)) & 3u;
                if (i < 16)
                    lo32[h] |= pair << (2 * i);
                else
                    hi32[h] |= pair << (2 * (i - 16));
            }
        }
#pragma unroll
        for (int h = 0; h < 4; h++)
            bits[h] = (uint64_t) lo32[h] | (uint64_t) hi32[h] << 32;
    }

    /* per lattice row: the word, its bits' count and the column bits; prefixes over the row's words */
    uint32_t rowId[4], rowCls[4], cnt[4], colCnt[4], colBits[4];
    bool rowExists[4];
    uint64_t mainBits[4];
#pragma unroll
    for (int h = 0; h < 4; h++)
    {
        const uint32_t y2 = 2 * y + (h & 1), z2 = 2 * z + (h >> 1);
        rowExists[h] = active && y2 <= L.topy && z2 <= L.z2Last;
        rowId[h] = (z2 - L.z2First) * L.rowsPerLayer + y2;
        rowCls[h] = L.rowClass(y2, z2);
        /* points beyond the row's end cannot exist (their cells do not), so the word needs no trimming */
        const uint64_t cm = rowCls[h] == 2 ? 0ull : L.columnMask(w);
        const uint64_t col = bits[h] & cm;
        const uint64_t topBit = w == (L.topx >> 6) ? 1ull << (L.topx & 63) : 0ull;
        colBits[h] = ((w == 0 && (col & 1ull)) ? LAT_FLAG_X0 : 0u) | ((col & topBit) ? LAT_FLAG_TOP : 0u);
        mainBits[h] = bits[h] & ~cm;
        cnt[h] = (uint32_t) __popcll(mainBits[h]);
        colCnt[h] = (uint32_t) __popcll(col);
    }
    /* inclusive sums over the lanes of the row of corners (w' <= w): counts up to 64 * nw <= 512 in 16-bit fields */
    uint32_t pa = cnt[0] | cnt[1] << 16, pb = cnt[2] | cnt[3] << 16, pc = colCnt[0] | colCnt[1] << 8 | colCnt[2] << 16 | colCnt[3] << 24;
    uint32_t ia = pa, ib = pb, ic = pc;
    for (uint32_t d = 1; d < nw; d++)
    {
        const uint32_t ta = (uint32_t) __shfl_up((int) pa, d, 64), tb = (uint32_t) __shfl_up((int) pb, d, 64),
                       tc = (uint32_t) __shfl_up((int) pc, d, 64);
        if (w >= d)
        {
            ia += ta;
            ib += tb;
            ic += tc;
        }
    }
    const uint32_t incl[4] = {ia & 0xFFFFu, ia >> 16, ib & 0xFFFFu, ib >> 16};
#pragma unroll
    for (int h = 0; h < 4; h++)
    {
        if (!rowExists[h])
            continue;
        L.words[(uint64_t) rowId[h] * nw + w] = LatWord{mainBits[h], incl[h] - cnt[h], colBits[h]};
        if (w == nw - 1)
            L.rowCounts[rowId[h]] = latticeRowCount(rowCls[h], incl[h], (ic >> (8 * h)) & 0xFFu);
    }
}

/* After the scan of the row counts, one thread per word: make the word's prefix an absolute output index and
 * give every word of a class-0/1 row the row's class-2 start and its two column bits. */
struct LatticePatchArgs
{
    Lattice L;
    uint32_t numWords;
};

__global__ __launch_bounds__(256) void latticePatchKernel(Lanes<LatticePatchArgs> lanes)
{
    const LatticePatchArgs A = lanes.a[blockIdx.y];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.numWords)
        return;
    const Lattice L = A.L;            /* a copy: the fields live in scalar registers, not behind kernel-argument loads */
    const uint32_t row = i / L.nw;
    const uint32_t z2 = row / L.rowsPerLayer + L.z2First, y2 = row % L.rowsPerLayer;
    const uint32_t rc = L.rowClass(y2, z2);
    const U3 rs = L.rowCounts[row];
    const U3 tot = *L.totals;
    const uint32_t off2 = tot.a + tot.b;
    const uint32_t mainBase = rc == 0 ? rs.a : (rc == 1 ? tot.a + rs.b : off2 + rs.c);
    /* bits 31 / 30 of word 0 / the top word keep their value through this kernel, so rows that straddle blocks are safe */
    const uint32_t x0 = L.words[(uint64_t) row * L.nw].flag & LAT_FLAG_X0;
    const uint32_t top = L.words[(uint64_t) row * L.nw + (L.topx >> 6)].flag & LAT_FLAG_TOP;
    L.words[i].prefix += mainBase;
    L.words[i].flag = (off2 + rs.c) | x0 | top;
}

/* 1.0f / x, correctly rounded, in three vector instructions where the compiler's division takes twelve: v_rcp_f32 and one
 * Newton step in fused arithmetic give the correctly rounded quotient for EVERY x with a biased exponent of 1 .. 252 --
 * checked exhaustively on gfx950 over all 2^32 inputs (tools/microbench/rcp_exact.hip: the only differences are zeros and
 * denormals, |x| >= 2^126, infinities and NaNs) -- and those take the division.  latticeVertices spent a third of an
 * iteration's vector instructions in it. */
__device__ __forceinline__ float exactRcp(float x)
{
    const uint32_t e = (__float_as_uint(x) >> 23) & 0xFFu;
    if (e - 1u < 252u)
    {
        const float r = __builtin_amdgcn_rcpf(x);
        return fmaf(r, fmaf(-x, r, 1.0f), r);
    }
    return 1.0f / x;
}

/* Positions (interp, kernels/marching.cl:130-138) and external keys of the existing points.  One wave per QUAD of lattice
 * rows -- (z2, y2) = (2 cz + pz, 2 cy + py): the four rows whose points hang off the corner row (cy, cz) -- lane = x2 within
 * a word.  The kernel was bound by memory latency times resident waves, not by bytes or instructions, so a wave carries as
 * much independent work as its registers allow: the four rows share the values of the corner row (five field loads per four
 * points instead of eight), the lattice words of a layer's two rows (8 words of each per trip) arrive with ONE coalesced load
 * -- lanes 0-31 hold row 2 cy's dwords, lanes 32-63 row 2 cy + 1's -- and are read out of it lane by lane into scalar
 * registers, and all of a trip's loads are requested before the first point is computed (a trip is 512 points: 255 cells).
 * Measured on cfg3, two buckets per launch: one row per wave 144 us, a pair 107, the quad 101 -- 517 MB of traffic at 5.1 TB/s. */
struct LatticeVerticesArgs
{
    Lattice L;
    FieldView F;
    float *outVertices;
    uint64_t *outKeys;
    uint32_t gox, goy, goz;
    uint64_t keyOffset;
    VertexTransform X;
    uint32_t numPairs;       /* quads: ceil(layers / 2) x ceil(rowsPerLayer / 2) */
};

/* XF: the scale / bias of ScaleBiasFilter for every bucket of the launch (1), for none (0), or as each bucket says (2: both
 * results computed and selected -- nine vector instructions of an iteration's ~40 instead of three) */
template<int XF>
__global__ __launch_bounds__(256) void latticeVerticesKernel(Lanes<LatticeVerticesArgs> lanes)
{
    const LatticeVerticesArgs A = lanes.a[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t quadId = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (quadId >= A.numPairs)
        return;
    const Lattice L = A.L;            /* a copy: the fields live in scalar registers, not behind kernel-argument loads */
    const FieldView F = A.F;
    float *const outVertices = A.outVertices;
    uint64_t *const outKeys = A.outKeys;
    const uint32_t gox = A.gox, goy = A.goy, goz = A.goz;
    const uint64_t keyOffset = A.keyOffset;
    const VertexTransform X = A.X;
    const uint32_t pairsPerLayer = (L.rowsPerLayer + 1) / 2;
    const uint32_t layers = L.z2Last - L.z2First + 1;
    const uint32_t slab = quadId / pairsPerLayer, cy = quadId % pairsPerLayer;      /* slab: the layers z2 = 2 cz and 2 cz + 1 */
    const uint32_t cz = (L.z2First >> 1) + slab;
    const bool hasY = 2 * cy + 1 < L.rowsPerLayer;      /* a layer's last row (y2 = top.y) is alone ... */
    const bool hasZ = 2 * slab + 1 < layers;            /* ... and so is the last layer */
    /* endpoint A of every point of the quad is a corner of the row (cy, cz); endpoint B is A + (px, py, pz) */
    const float *fieldB[2][2];
#pragma unroll
    for (int pz = 0; pz < 2; pz++)
#pragma unroll
        for (int py = 0; py < 2; py++)
            fieldB[pz][py] = F.field + (uint64_t) (cy + (hasY ? py : 0) + F.zStride * (cz + (hasZ ? pz : 0)) + (uint32_t) F.zBias) * F.pitch;
    const float *const field0 = fieldB[0][0];
    const uint32_t px = lane & 1;
    const uint32_t rowDwords = 4 * L.nw;
    const uint32_t *wordsOf[2];      /* per layer: row y2 = 2 cy's dwords; row 2 cy + 1's follow */
#pragma unroll
    for (int pz = 0; pz < 2; pz++)
        wordsOf[pz] = (const uint32_t *) (L.words + (uint64_t) ((2 * slab + (hasZ ? pz : 0)) * L.rowsPerLayer + 2 * cy) * L.nw);
    /* interp (kernels/marching.cl:130-138), scale / bias, the vertex and -- for an external one -- its key.  Endpoint A =
     * owner corner, B = A + (px, py, pz): A has the lower local corner id in every cell */
    auto emit = [&](uint32_t x2, uint32_t cx, uint32_t ex, uint32_t ey, uint32_t ez, uint32_t idx, float isoA, float isoB, bool withKey)
    {
        const float inv = exactRcp(isoA - isoB);
        const float t = isoA * inv;
        float vx = fmaf(t, (float) ex, (float) (cx + gox));
        float vy = fmaf(t, (float) ey, (float) (cy + goy));
        float vz = fmaf(t, (float) ez, (float) (cz + goz));
        if (XF == 2 ? (bool) X.enabled : XF == 1)
        {
            vx = fmaf(vx, X.scale, X.bx);
            vy = fmaf(vy, X.scale, X.by);
            vz = fmaf(vz, X.scale, X.bz);
        }
        outVertices[3 * (uint64_t) idx + 0] = vx;
        outVertices[3 * (uint64_t) idx + 1] = vy;
        outVertices[3 * (uint64_t) idx + 2] = vz;
        if (withKey)
            outKeys[idx] = (((uint64_t) (2 * cz + ez) << (2 * KEY_AXIS_BITS)) | ((uint64_t) (2 * cy + ey) << KEY_AXIS_BITS) | (uint64_t) x2) + keyOffset;
    };
    constexpr int G = 8;
    for (uint32_t w0 = 0; w0 < L.nw; w0 += G)
    {
        /* dword (lane % 32) of the trip's eight words of row y2 = 2 cy (lanes 0-31) and 2 cy + 1 (lanes 32-63), clamped */
        const uint32_t dw = min(4 * w0 + (lane & 31u), rowDwords - 1) + ((lane >> 5) != 0 && hasY ? rowDwords : 0u);
        const uint32_t latDword[2] = {wordsOf[0][dw], wordsOf[1][dw]};
        float iso0[G], iso1[2][2][G];
#pragma unroll
        for (int j = 0; j < G; j++)
        {
            /* every lane loads (clamped inside the row), so the loads do not wait on the masks; checking the words for
             * emptiness first was measured: -7 % on surface-like data, +8 % on the noise cloud (exposed latency) */
            const uint32_t w = min(w0 + j, L.nw - 1);
            const uint32_t cx = min(w * 32 + (lane >> 1), L.cw - px);
            iso0[j] = field0[cx];
#pragma unroll
            for (int pz = 0; pz < 2; pz++)
#pragma unroll
                for (int py = 0; py < 2; py++)
                    iso1[pz][py][j] = fieldB[pz][py][cx + px];
        }
#pragma unroll
        for (int j = 0; j < G; j++)
        {
            if (w0 + j >= L.nw)
                break;
            const uint32_t x2 = (w0 + j) * 64 + lane;
            const uint32_t cx = x2 >> 1;
#pragma unroll
            for (int pz = 0; pz < 2; pz++)
            {
                if (pz == 1 && !hasZ)
                    break;
#pragma unroll
                for (int py = 0; py < 2; py++)
                {
                    if (py == 1 && !hasY)
                        break;
                    const uint32_t y2 = 2 * cy + py, z2 = 2 * cz + pz;
                    const uint32_t cls = L.rowClass(y2, z2);
                    const uint32_t at = 32 * py + 4 * j;
                    const uint64_t exists = (uint64_t) readLane(latDword[pz], at) | (uint64_t) readLane(latDword[pz], at + 1) << 32;
                    const uint32_t prefix = readLane(latDword[pz], at + 2);
                    if (!((exists >> lane) & 1))
                        continue;
                    /* (a class-0/1 row's two class-2 points, x2 = 0 and x2 = top.x, are not in the mask: see below) */
                    const uint32_t idx = prefix + (uint32_t) __popcll(exists & ((1ull << lane) - 1));
                    emit(x2, cx, px, (uint32_t) py, (uint32_t) pz, idx, iso0[j], iso1[pz][py][j], cls != 0);
                }
            }
        }
    }
    /* The class-2 points inside class-0/1 rows -- x2 = 0 and x2 = top.x of each of the quad's four rows, where the row's flag
     * word says they exist (the same in every word of the row, latticePatchKernel) -- once per wave, a lane per candidate,
     * instead of two comparisons and their scalar bookkeeping in each of the loop's iterations (24 per wave on cfg3: the
     * kernel issued as many scalar as vector instructions, 63 % of the CU's scalar unit). */
    if (lane < 8)
    {
        const uint32_t r = lane >> 1, py = r & 1u, pz = r >> 1, top = lane & 1u;
        const uint32_t y2 = 2 * cy + py, z2 = 2 * cz + pz;
        if ((py == 0 || hasY) && (pz == 0 || hasZ) && L.rowClass(y2, z2) != 2)
        {
            const uint32_t flag = (pz ? wordsOf[1] : wordsOf[0])[(py ? rowDwords : 0u) + 3u];
            if (flag & (top ? LAT_FLAG_TOP : LAT_FLAG_X0))
            {
                const uint32_t x2 = top ? L.topx : 0u, cx = x2 >> 1;            /* top.x is even: px = 0 */
                const uint32_t idx = (flag & LAT_FLAG_INDEX) + (top ? flag >> 31 : 0u);     /* columnVertex, top a lane's */
                const float *const rowB = F.field + (uint64_t) (cy + py + F.zStride * (cz + pz) + (uint32_t) F.zBias) * F.pitch;
                emit(x2, cx, 0u, py, pz, idx, field0[cx], rowB[cx], true);
            }
        }
    }
}

/* Lattice weld: the occupied cells of the batch in cell-linear order with each cell's first index slot.
 * One wave per row of cells; a row's first cell / index slot come from the exclusive scan of the row totals,
 * positions inside the row from a ballot rank and a wave scan. */
struct CompactRowCellsArgs
{
    const uint8_t *codes;
    uint32_t cw, ch, z0, zFirst;
    const U3 *rowStarts;
    const uchar2 *countTable;
    uint2 *cells, *viStart;
    uint32_t numRows;
};

__global__ __launch_bounds__(256) void compactRowCellsKernel(Lanes<CompactRowCellsArgs> lanes)
{
    const CompactRowCellsArgs A = lanes.a[blockIdx.y];
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= A.numRows)
        return;
    const uint8_t *const codes = A.codes;
    const uint32_t cw = A.cw, ch = A.ch, z0 = A.z0, zFirst = A.zFirst;
    const U3 *const rowStarts = A.rowStarts;
    const uchar2 *const countTable = A.countTable;
    uint2 *const cells = A.cells, *const viStart = A.viStart;
    const uint32_t y = r % ch, z = r / ch + zFirst;
    const uint8_t *row = codes + ((uint64_t) (z - z0) * ch + y) * cw;
    const U3 start = rowStarts[r];
    uint32_t cellBase = start.a, indexBase = start.c;
    for (uint32_t x0 = 0; x0 < cw; x0 += 64)
    {
        const uint32_t x = x0 + lane;
        const uint32_t code = x < cw ? row[x] : 0u;
        const uint32_t ni = code != 0 ? countTable[code].y : 0u;
        const uint64_t occ = __ballot(code != 0);
        const uint32_t incl = waveInclusiveScan(ni);
        if (code != 0)
        {
            const uint32_t pos = cellBase + popcBelow(occ);
            cells[pos] = make_uint2(x | (y << 16), z | (code << 16));     /* the code rides along: one dependent load less */
            viStart[pos] = make_uint2(0u, indexBase + incl - ni);
        }
        cellBase += (uint32_t) __popcll(occ);
        indexBase += readLane(incl, 63);
    }
}

/* One thread per occupied cell: look up the welded index of each of the cell's vertices, then emit its
 * triangles (the index half of generateElements + reindex).
 *
 * The cell's 19 possible vertices lie in 9 lattice rows (y2, z2) = (2y + 0..2, 2z + 0..2) at x2 = 2x + 0..2, and
 * x2 = 2x + 2 still ranks inside the word of 2x (a full-word popcount when it is the next word's bit 0), so the
 * lookup is nine independent 16-byte loads issued together, then 19 unrolled edge tests -- vertex slots follow
 * edge ids (makeTables), so no per-code key table is needed.
 *
 * A block's cells are consecutive in the compacted list, so their index ranges are one contiguous span of the
 * output: it is assembled in LDS and written with fully coalesced stores. */
struct LatticeTrianglesArgs
{
    Lattice L;
    DevTables T;
    const uint2 *cells, *viStart;
    uint32_t *indices;
    const U3 *batchTotals;
};

__global__ __launch_bounds__(256) void latticeTrianglesKernel(Lanes<LatticeTrianglesArgs> lanes)
{
    __shared__ uint32_t sIdx[256][MAX_CELL_VERTICES];
    __shared__ uint16_t sRef[256 * MAX_CELL_INDICES];   /* thread * 13 + vertex slot: 18 KB instead of 36 KB of indices */
    __shared__ uint32_t sSpan;
    const LatticeTrianglesArgs A = lanes.a[blockIdx.y];
    const Lattice L = A.L;            /* a copy: the fields live in scalar registers, not behind kernel-argument loads */
    const DevTables T = A.T;
    const uint2 *const cells = A.cells, *const viStart = A.viStart;
    uint32_t *const indices = A.indices;
    const uint32_t numCells = A.batchTotals->a;         /* grid covers the host's count; the device value rules */
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (blockIdx.x * blockDim.x >= numCells)
        return;
    const uint32_t blockBase = viStart[blockIdx.x * blockDim.x].y;
    if (gid < numCells)
    {
        const uint2 cell = cells[gid];
        const uint32_t x = cell.x & 0xFFFFu, y = cell.x >> 16, z = cell.y & 0xFFFFu;
        const uint32_t code = cell.y >> 16;                  /* packed by compactRowCellsKernel */
        const uint32_t local = viStart[gid].y - blockBase;
        /* the whole record at once (index count in word 3, index bytes in words 4..12), together with the nine words */
        const uint4 *rec4 = (const uint4 *) T.rec + code * 4;
        const uint4 r0 = rec4[0], r1 = rec4[1], r2 = rec4[2];
        const uint32_t r12 = T.rec[code * 16 + 12];
        const uint32_t ni = r0.w >> 8;
        /* the nine rows' words */
        const uint32_t wIdx = (2 * x) >> 6, sh = (2 * x) & 63;
        LatWord wd[9];
        bool rowFlagged[9];
#pragma unroll
        for (int r = 0; r < 9; r++)
        {
            const uint32_t y2 = 2 * y + (r % 3), z2 = 2 * z + (r / 3);
            const uint32_t row = (z2 - L.z2First) * L.rowsPerLayer + y2;
            wd[r] = L.words[(uint64_t) row * L.nw + wIdx];
            rowFlagged[r] = L.rowFlagged(y2, z2);
        }
        /* bits of the word below x2 = 2x + px */
        uint64_t below[3];
        below[0] = (1ull << sh) - 1;
        below[1] = (2ull << sh) - 1;
        below[2] = sh == 62 ? ~0ull : (4ull << sh) - 1;
        const bool atX0 = x == 0, atTop = 2 * x + 2 == L.topx;
        uint32_t slot = 0;
#pragma unroll
        for (int e = 0; e < NUM_EDGES; e++)
        {
            const EdgePoint p = edgePoint(e);
            const int px = p.px, r = p.q;
            if (edgeBit(code, p.a, p.b))
            {
                uint32_t idx = wd[r].prefix + (uint32_t) __popcll(wd[r].mask & below[px]);
                if (px == 0 && atX0 && !rowFlagged[r])
                    idx = columnVertex<false>(wd[r].flag);
                if (px == 2 && atTop && !rowFlagged[r])
                    idx = columnVertex<true>(wd[r].flag);
                sIdx[threadIdx.x][slot++] = idx;
            }
        }
        /* a reference is the word index of the vertex's welded index inside sIdx: one LDS read resolves it */
        const uint32_t first = threadIdx.x * MAX_CELL_VERTICES;
        const uint32_t iws[9] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r12};
#pragma unroll
        for (uint32_t q = 0; q < 9; q++)
        {
            if (4 * q >= ni)
                break;
            const uint32_t iw = iws[q];
            const uint32_t left = ni - 4 * q;
            sRef[local + 4 * q] = (uint16_t) (first + (iw & 0xFF));
            if (left > 1) sRef[local + 4 * q + 1] = (uint16_t) (first + ((iw >> 8) & 0xFF));
            if (left > 2) sRef[local + 4 * q + 2] = (uint16_t) (first + ((iw >> 16) & 0xFF));
            if (left > 3) sRef[local + 4 * q + 3] = (uint16_t) (first + (iw >> 24));
        }
        if (gid == numCells - 1 || threadIdx.x == blockDim.x - 1)
            sSpan = local + ni;
    }
    __syncthreads();
    const uint32_t span = sSpan;
    /* four positions per thread and trip, so that the two dependent LDS reads of a position overlap the others' */
    const uint32_t *flat = &sIdx[0][0];
    for (uint32_t k0 = 0; k0 < span; k0 += 4 * 256)
    {
        uint32_t ref[4], val[4];
#pragma unroll
        for (int u = 0; u < 4; u++)
        {
            const uint32_t k = k0 + 256 * u + threadIdx.x;
            ref[u] = k < span ? sRef[k] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            val[u] = flat[ref[u]];
#pragma unroll
        for (int u = 0; u < 4; u++)
        {
            const uint32_t k = k0 + 256 * u + threadIdx.x;
            if (k < span)
                indices[blockBase + k] = val[u];
        }
    }
}

/* The same emission without the compacted cell list: one wave per ROW of cells, lane = cell x, 64 cells at a time.  The
 * code bytes are one coalesced read, the row's first index slot comes from the scan of the row totals and a cell's slot
 * from a wave scan of the per-code index counts -- so the (cell, first slot) records that compactRowCellsKernel wrote and
 * latticeTrianglesKernel read back (16 bytes per occupied cell each way, and a dependent load in front of everything
 * else) do not exist.  The nine lattice rows are the same for the whole wave.  Index order is unchanged: rows in (z, y)
 * order, cells by x, a cell's indices in table order.  Each wave stages its own span in LDS; no workgroup barrier. */
struct LatticeTrianglesRowArgs
{
    Lattice L;
    CodeView C;
    DevTables T;
    const U3 *rowCounts, *rowStarts;
    uint32_t zFirst;
    uint32_t *indices;
    uint32_t numRows;
    uint32_t *trash;         /* a word nobody reads: where the stores of a chunk without indices go */
};

/* Software-pipelined over the chunks of a row: nothing chunk n + 1 needs is requested after chunk n's stores.  Vector loads
 * and stores retire in order (one counter, vmcnt), so a load issued behind a chunk's stores is usable only when all of them
 * have reached the L2.  Here the loads of chunk n + 1 (its code records; the code bytes of chunk n + 2) are issued BEFORE the
 * stores of chunk n, and every chunk issues a number of stores the compiler can count (three per quarter of the wave, a fourth
 * for a quarter of more than 192 indices; one of more than 256 drains), so the wait in front of chunk n + 1 is `vmcnt(12)`:
 * chunk n's stores stay in flight.  (A path through the loop without stores -- an empty chunk skipped, a predicated store --
 * would make that wait a full one again, which is why positions past a quarter's end store its last index once more and an
 * empty quarter stores to a word nobody reads.)  The
 * lattice words of the row's nine lattice rows are staged once in LDS (dynamic: 4 x 9 x nw x 16 bytes) instead of nine
 * 16-byte loads per cell; a vertex index is its row's word prefix plus the mask bits below its x2, counted once per row
 * (not per edge); the references go out four or eight bytes at a time.  Measured on cfg3 (two buckets per launch): 216 -> 195 us,
 * 3.16 -> 2.90 ms per step (profiles/NOTES_r04.md section 9). */
__global__ __launch_bounds__(256) void latticeTrianglesRowKernel(Lanes<LatticeTrianglesRowArgs> lanes)
{
    const LatticeTrianglesRowArgs A = lanes.a[blockIdx.y];
    const Lattice L = A.L;
    const CodeView C = A.C;
    const DevTables T = A.T;
    const U3 *const rowCounts = A.rowCounts, *const rowStarts = A.rowStarts;
    const uint32_t zFirst = A.zFirst, numRows = A.numRows;
    uint32_t *const indices = A.indices, *const trash = A.trash;
    __shared__ uint32_t sIdx[4][64][MAX_CELL_VERTICES];
    __shared__ uint8_t sRef[4][64 * MAX_CELL_INDICES];
    extern __shared__ uint4 sLat[];                 /* [4][9][nw] */
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
    if (r >= numRows)
        return;
    /* everything the row needs that does not depend on another load is requested at once: the row's totals, its first
     * code bytes and the lattice words (an empty row returns with those requests in flight; the rows route is the dense one) */
    const uint32_t y = r % L.ch, z = r / L.ch + zFirst;
    const uint8_t *codeRow = C.codes + ((uint64_t) (z - C.z0) * C.ch + y) * C.cw;
    const uint32_t nw = L.nw, cw = L.cw;
    const uint32_t occupied = rowCounts[r].a;
    uint32_t indexBase = rowStarts[r].c;
    uint32_t c0 = lane < cw ? codeRow[lane] : 0u;
    uint32_t c1 = lane + 64 < cw ? codeRow[lane + 64] : 0u;
    uint4 *const myLat = sLat + wv * 9 * nw;
    bool rowFlagged[9];
#pragma unroll
    for (int q = 0; q < 9; q++)
    {
        const uint32_t y2 = 2 * y + (q % 3), z2 = 2 * z + (q / 3);
        rowFlagged[q] = L.rowFlagged(y2, z2);
    }
    /* the 9 x nw lattice words, 64 per request: entry e is word e % nw of row e / nw (nw <= 64: the division is a multiply) */
    const uint32_t entries = 9 * nw, recip = (65536u + nw - 1) / nw;
    auto latWord = [&](const uint32_t e) -> const uint4 *
    {
        const uint32_t q = (e * recip) >> 16, w = e - q * nw;
        const uint32_t qz = (q * 11u) >> 5, qy = q - 3u * qz;
        return (const uint4 *) (L.words + (uint64_t) ((2 * z + qz - L.z2First) * L.rowsPerLayer + 2 * y + qy) * nw + w);
    };
    const uint32_t e0 = min(lane, entries - 1), e1 = min(lane + 64, entries - 1);
    const uint4 w0 = *latWord(e0), w1 = *latWord(e1);
    if (__builtin_amdgcn_readfirstlane(occupied) == 0)
        return;
    const uint4 *rec4 = (const uint4 *) T.rec;
    uint4 n1 = rec4[c0 * 4 + 1], n2 = rec4[c0 * 4 + 2], n3 = rec4[c0 * 4 + 3];
    myLat[e0] = w0;
    myLat[e1] = w1;
    for (uint32_t e = 128 + lane; e < entries; e += 64)
        myLat[e] = *latWord(e);
    uint32_t (*myIdx)[MAX_CELL_VERTICES] = sIdx[wv];
    uint8_t *myRef = sRef[wv];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    /* a class-0/1 row's flag word is the same in all of its words (latticePatchKernel) */
    uint32_t rowFlag[9];
#pragma unroll
    for (int q = 0; q < 9; q++)
        rowFlag[q] = __builtin_amdgcn_readfirstlane(myLat[q * nw].w);
    __builtin_amdgcn_s_waitcnt(0x0F70);            /* vmcnt(0): the loop is entered with nothing in flight, so that the waits
                                                    * inside it are the steady state's, not the first chunk's */
    for (uint32_t x0 = 0; x0 < cw; x0 += 64)
    {
        const uint32_t x = x0 + lane;
        const uint32_t code = c0;
        const uint4 r1 = n1, r2 = n2, r3 = n3;
        /* the next chunk's records and the code bytes of the one after it */
        c0 = c1;
        c1 = x + 128 < cw ? codeRow[x + 128] : 0u;
        n1 = rec4[c0 * 4 + 1];
        n2 = rec4[c0 * 4 + 2];
        n3 = rec4[c0 * 4 + 3];
        const uint32_t ni = r3.w >> 8;             /* code 0 (not occupied, or past the row's end): an all-zero record */
        const uint32_t incl = waveInclusiveScan(ni);
        const uint32_t span = readLane(incl, 63);
        const uint32_t local = incl - ni;
        if (code != 0)
        {
            const uint32_t wIdx = (2 * x) >> 6, sh = (2 * x) & 63;
            const uint64_t below0 = (1ull << sh) - 1, below1 = (2ull << sh) - 1;
            const bool atX0 = x == 0, atTop = 2 * x + 2 == L.topx;
            uint32_t base[9], two[9];
#pragma unroll
            for (int q = 0; q < 9; q++)
            {
                const bool throughCorners = (q % 3) != 1 && (q / 3) != 1;
                const uint4 wd = myLat[q * nw + wIdx];
                const uint64_t mask = (uint64_t) wd.x | (uint64_t) wd.y << 32;
                base[q] = wd.z + (uint32_t) __popcll(mask & (throughCorners ? below1 : below0));
                two[q] = throughCorners ? 0u : (uint32_t) (mask >> sh) & 3u;
            }
            const uint32_t used = r3.z;
            uint32_t *dst = myIdx[lane];
#pragma unroll
            for (int e = 0; e < NUM_EDGES; e++)
            {
                const EdgePoint p = edgePoint(e);
                const int px = p.px, q = p.q;
                const bool throughCorners = (q % 3) != 1 && (q / 3) != 1;
                if (used & (1u << e))
                {
                    uint32_t idx = base[q];
                    if (!throughCorners && px == 1)
                        idx += two[q] & 1u;
                    if (!throughCorners && px == 2)
                        idx += (uint32_t) __popc(two[q]);
                    if (px == 0 && atX0 && !rowFlagged[q])
                        idx = columnVertex<false>(rowFlag[q]);
                    if (px == 2 && atTop && !rowFlagged[q])
                        idx = columnVertex<true>(rowFlag[q]);
                    *dst++ = idx;
                }
            }
            const uint32_t first4 = (lane & 15u) * (MAX_CELL_VERTICES * 0x01010101u);
            const uint32_t iws[9] = {r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w, r3.x};
            uint8_t *const ref = myRef + local;
            const uint32_t whole = ni >> 2;
            /* two words per store where two are whole (an unaligned 8-byte LDS store costs what a 4-byte one does) */
#pragma unroll
            for (uint32_t q = 0; q < 8; q += 2)
            {
                if (q + 1 < whole)
                {
                    const uint64_t v = (uint64_t) (iws[q] + first4) | (uint64_t) (iws[q + 1] + first4) << 32;
                    __builtin_memcpy(ref + 4 * q, &v, 8);
                }
                else if (q < whole)
                {
                    const uint32_t v = iws[q] + first4;
                    __builtin_memcpy(ref + 4 * q, &v, 4);
                }
            }
            if (8 < whole)
            {
                const uint32_t v = iws[8] + first4;
                __builtin_memcpy(ref + 32, &v, 4);
            }
            const uint32_t rest = ni & 3u, tail = r3.y + first4;
            if (rest > 0) ref[4 * whole] = (uint8_t) tail;
            if (rest > 1) ref[4 * whole + 1] = (uint8_t) (tail >> 8);
            if (rest > 2) ref[4 * whole + 2] = (uint8_t) (tail >> 16);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        /* The write-out, one QUARTER of the wave (16 cells, whose 16 x 13 slots a reference byte can address) at a time: a
         * quarter's positions are the interval between two wave-uniform bounds, so a position costs an add, a clamp and the
         * two LDS reads.  Every lane stores in the three trips every quarter makes (192 positions; 16 cells hold 189 on the
         * uniform cloud): a position past the quarter's end is its last once more (same value, same address), an empty
         * quarter stores to a word nobody reads -- so that the number of stores does not depend on the data. */
        const uint32_t bound[5] = {0u, readLane(incl, 15), readLane(incl, 31), readLane(incl, 47), span};
        uint32_t *const out = indices + indexBase;
        bool drain = false;
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const uint32_t lo = bound[i], hi = bound[i + 1];
            const uint32_t *const slots = &myIdx[16 * i][0];
            const uint32_t last = hi != lo ? hi - 1 : lo;
            uint32_t *const dstq = hi != lo ? out : trash - lo;
            const uint32_t refMask = hi != lo ? 0xFFu : 0u;      /* an empty quarter's reference byte is stale: slot 0 then */
            uint32_t k[3], val[3];
#pragma unroll
            for (int u = 0; u < 3; u++)
            {
                k[u] = min(lo + 64 * u + lane, last);
                val[u] = myRef[k[u]] & refMask;
            }
#pragma unroll
            for (int u = 0; u < 3; u++)
                val[u] = slots[val[u]];
#pragma unroll
            for (int u = 0; u < 3; u++)
                dstq[k[u]] = val[u];
            if (hi - lo > 192)
            {
                const uint32_t k3 = min(lo + 192 + lane, last);
                dstq[k3] = slots[myRef[k3]];
            }
            if (hi - lo > 256)
            {
#pragma unroll 1
                for (uint32_t k0 = lo + 256 + lane; k0 < hi; k0 += 64)
                    out[k0] = slots[myRef[k0]];
                drain = true;
            }
        }
        if (drain)
            __builtin_amdgcn_s_waitcnt(0x0F70);    /* vmcnt(0): the count of those stores is not known at compile time */
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        indexBase += span;
    }
}

} // namespace

#endif
