/*
 * The host arithmetic of marching (marching.hip): the sizes of an object's buffers, the geometry of the half lattice of a
 * ship-out with the launch counts that follow from it, the rules that choose a weld, a mask kernel and a triangle route,
 * the sort weld's key layout, and how a swathe that overflows the mesh memory is cut into runs of slices.  Plain C++17, no
 * HIP: a stand-alone program (marchingplan_test.cpp) runs it without a GPU.
 */
#ifndef MLSGPU_MARCHINGPLAN_HPP
#define MLSGPU_MARCHINGPLAN_HPP

#include "../../include/mlsgpu_hip.h"

#include <algorithm>
#include <cstdint>

namespace mlsgpu
{

enum
{
    MAX_CELL_VERTICES = 13,
    MAX_CELL_INDICES = 36
};

/* The half lattice of cells z in [zTop, zMax) of a swathe of W x H corners (marching_lattice.hpp): what the device's
 * `Lattice` holds, the rows the launches walk and how many workgroups' worth of them there are. */
struct LatticeDims
{
    uint32_t nw;             /* 64-bit words per row */
    uint32_t rowsPerLayer;   /* 2H - 1 */
    uint32_t topx, topy;     /* 2(W-1), 2(H-1) */
    uint32_t z2First;        /* 2 * zTop: first layer, also top.z */
    uint32_t z2Last;         /* 2 * zMax: last layer */
    uint32_t cw, ch;         /* cells per row / rows of cells */
    uint32_t numRows, cornerRows, cellRows;     /* rows of the lattice, of corners, of cells */

    LatticeDims(uint32_t W, uint32_t H, uint32_t zTop, uint32_t zMax)
        : nw((2 * W - 1 + 63) / 64), rowsPerLayer(2 * H - 1), topx(2 * (W - 1)), topy(2 * (H - 1)), z2First(2 * zTop),
          z2Last(2 * zMax), cw(W - 1), ch(H - 1), numRows((2 * (zMax - zTop) + 1) * rowsPerLayer),
          cornerRows((zMax - zTop + 1) * H), cellRows((zMax - zTop) * ch)
    {
    }
    LatticeDims() : LatticeDims(1, 1, 0, 0) {}

    uint32_t layers() const { return z2Last - z2First + 1; }
    bool fits(uint64_t latRowsMax, uint32_t latWords) const { return numRows <= latRowsMax && nw <= latWords; }
    /* latticePatchKernel: a thread per word */
    uint32_t numWords() const { return numRows * nw; }
    /* latticeVerticesKernel: a wave per quad of rows, ceil(layers / 2) x ceil(rowsPerLayer / 2) */
    uint32_t numQuads() const { return (layers() + 1) / 2 * ((rowsPerLayer + 1) / 2); }
    /* workgroups (four waves) of a mask kernel: latticeMaskKernel takes a row of corners per wave, latticeMaskWordKernel
     * (a thread per word, nw <= 64) 64 / nw of them */
    uint32_t maskGroups(bool byRows) const { return (cornerRows + rowsPerGroup(byRows) - 1) / rowsPerGroup(byRows); }
    uint32_t rowsPerGroup(bool byRows) const { return byRows ? 4u : 4u * (64u / nw); }
};

/* What the constructor works out from its arguments (src/marching.cpp:273-284) */
struct MarchingSizes
{
    uint32_t imageWidth, imageHeight, zStride, maxSwathe;
    uint64_t swatheCells, vertexSpace, indexSpace, fieldRows;
    bool legacyBuffers;      /* false: every bucket fits one swathe, the sort weld is never needed */
    uint64_t latRowsMax;
    uint32_t latWords;

    MarchingSizes(uint32_t maxWidth, uint32_t maxHeight, uint32_t maxDepth, uint32_t swatheLimit, uint64_t meshMemory,
                  const uint32_t alignment[3])
    {
        imageWidth = (maxWidth + alignment[0] - 1) / alignment[0] * alignment[0];
        imageHeight = zStride = (maxHeight + alignment[1] - 1) / alignment[1] * alignment[1];
        maxSwathe = std::min(swatheLimit, maxDepth) / alignment[2] * alignment[2];
        swatheCells = (uint64_t) (maxWidth - 1) * (maxHeight - 1) * maxSwathe;
        const uint64_t meshCells = meshMemory / MLSGPU_MARCHING_MAX_CELL_BYTES;
        vertexSpace = meshCells * MAX_CELL_VERTICES;
        indexSpace = meshCells * MAX_CELL_INDICES;
        /* image height imageHeight * (maxSwathe + 1) (src/marching.cpp:380-381), plus the slack a
         * generator may write when the last swathe is padded up to its Z alignment (src/marching.h:236-237) */
        fieldRows = (uint64_t) imageHeight * (maxSwathe + 1 + alignment[2]);
        legacyBuffers = maxSwathe < maxDepth;           /* some bucket may need more than one swathe */
        const LatticeDims widest(maxWidth, maxHeight, 0, maxSwathe);
        latRowsMax = (uint64_t) widest.layers() * widest.rowsPerLayer;
        latWords = widest.nw;
    }
};

/* latticeMaskKernel (a wave per row of corners) instead of latticeMaskWordKernel (a thread per word) for a ship-out: rows
 * wider than 2 048 corners have more words than a wave has lanes.  `forced`: MLSGPU_HIP_LATTICE_MASK_ROWS, for A/B. */
inline bool maskByRows(uint32_t nw, bool forced)
{
    return forced || nw > 64;
}

/* Two routes to the same index list, chosen per bucket.  By ROWS (one wave per row of cells, no compacted cell list): no
 * compactRowCells launch and 32 bytes per occupied cell less traffic, but a wave per row whatever it holds -- the
 * faster one when most cells are occupied (cfg3 noise cloud, 85 %: 4.2 -> 3.6 ms per step).  By CELLS (compact, then
 * one thread per occupied cell): time follows the surface, 0.70 against 1.31 ms per step on the shells cloud
 * (~6 % occupied).
 * Rows when at least a quarter of the cells are occupied (the rows kernel walks every cell, the cells route pays a
 * compaction first): the slabs of the 1024^3 cloud, a third to a half occupied, 10.83 ms per step by cells and 10.60 by
 * rows; the shells cloud (under a sixth) 0.51 against 0.90 ms of emission.
 * The rows kernel stages 9 x nw lattice words per wave in LDS and divides by nw with a 16-bit reciprocal: a lattice wider
 * than 64 words -- 2047 cells -- takes the cells route whatever its density.
 * `forced`: MLSGPU_HIP_TRIANGLES_BY_CELLS, 0 (rows) or 1 (cells); negative when it is not set. */
inline bool trianglesByCells(uint32_t nw, uint32_t occupiedCells, uint32_t cellRows, uint32_t cw, int forced)
{
    const uint32_t rowsFactor = 4;
    if (nw > 64)
        return true;
    if (forced >= 0)
        return forced != 0;
    return (uint64_t) occupiedCells * rowsFactor < (uint64_t) cellRows * cw;
}

enum WeldRoute
{
    WELD_LATTICE,
    WELD_SORT,
    WELD_NONE        /* several swathes, but the object was created for one: the caller's MLSGPU_ERR_LENGTH */
};

/* One swathe covers the bucket: weld from the resident field without sorting.  Otherwise (or when forced with
 * MLSGPU_HIP_WELD=sort, if the object has the buffers) the reference's generate + sort + compact structure is used. */
inline WeldRoute weldRoute(uint32_t depth, uint32_t maxSwathe, bool legacyBuffers, bool forceSort)
{
    if (depth <= maxSwathe && !(forceSort && legacyBuffers))
        return WELD_LATTICE;
    return legacyBuffers ? WELD_SORT : WELD_NONE;
}

inline uint32_t bitsFor(uint32_t maxValue)
{
    uint32_t b = 1;
    while ((maxValue >> b) != 0)
        b++;
    return b;
}

/* the generate-time layout of the sort weld's keys: only as many bits as the bucket's doubled local coordinates need */
struct KeyBits
{
    uint32_t bx, by, bz;
    uint32_t bits() const { return bx + by + bz + 1; }
    bool wideKeys() const { return bits() > 32; }
};

inline KeyBits keyLayout(const uint32_t size[3])
{
    return KeyBits{bitsFor(2 * (size[0] - 1)), bitsFor(2 * (size[1] - 1)), bitsFor(2 * (size[2] - 1))};
}

/* (vertices, indices) of one slice of cells */
struct SliceCounts
{
    uint32_t vertices, indices;
};

/* The next run of slices of a swathe that is too big on its own (src/marching.cpp:652-701): with hist[z] the counts of
 * slice z and `offsets` what is buffered, the end of the run [first, end) that fits behind the buffered elements or, if
 * not even slice `first` does, of the run that fits once they are flushed.  `first` itself when that slice alone exceeds
 * the space (or the range is empty). */
inline uint32_t sliceRun(const SliceCounts *hist, uint32_t first, uint32_t last, const uint32_t offsets[2], uint64_t vertexSpace,
                         uint64_t indexSpace)
{
    for (int flushed = 0; flushed < 2; flushed++)
    {
        uint64_t c0 = flushed ? 0 : offsets[0], c1 = flushed ? 0 : offsets[1];
        uint32_t end = first;
        while (end < last && c0 + hist[end].vertices <= vertexSpace && c1 + hist[end].indices <= indexSpace)
        {
            c0 += hist[end].vertices;
            c1 += hist[end].indices;
            end++;
        }
        if (end > first)
            return end;
    }
    return first;
}

} // namespace mlsgpu

#endif
