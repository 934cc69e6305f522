/*
 * The host arithmetic of the sparse triangle grid (meshgrid.hpp) under the deviation and the self-intersection report, for a
 * plain compiler: no HIP, so that tests/test_meshgrid_plan.py can ask a sanitized stand-alone driver (meshgridplan_test.cpp)
 * what the stages would decide.  What runs on both sides is marked MLSGPU_HD.
 *
 * Neither report depends on anything here -- their contracts hold for every cell size -- so no test of the reports notices
 * a change of this plan; the plan's own tests do.
 */
#ifndef MLSGPU_AMD_MESHGRIDPLAN_HPP
#define MLSGPU_AMD_MESHGRIDPLAN_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define MLSGPU_HD __host__ __device__
#else
#define MLSGPU_HD
#endif

namespace mlsgpu
{

MLSGPU_HD inline uint32_t bitLength(uint64_t v)
{
    uint32_t b = 0;
    while (v != 0)
    {
        b++;
        v >>= 1;
    }
    return b;
}

/* e with 2^e <= M < 2^(e + 1) from the bits of a double M > 0 (a subnormal's true exponent) */
MLSGPU_HD inline int exponentOfDoubleBits(uint64_t bits)
{
    const int field = (int) (bits >> 52);
    if (field != 0)
        return field - 1023;
    int top = 0;
    for (uint64_t m = bits; m > 1; m >>= 1)
        top++;
    return top - 1074;
}

/* 2^k as a double, for a k that gives a normal one */
MLSGPU_HD inline double powerOfTwo(int k)
{
    const long long bits = (long long) (1023 + k) << 52;
    double d;
    __builtin_memcpy(&d, &bits, sizeof(d));
    return d;
}

/* floats to integers of the same order (and back): what atomicMin / atomicMax take */
MLSGPU_HD inline uint32_t orderedBits(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
inline float fromOrdered(uint32_t o)
{
    const uint32_t bits = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    std::memcpy(&f, &bits, sizeof(f));
    return f;
}

/* cells per axis: 3 * 21 bits pack a cell, which the self-intersection report's owning-cell rule needs (and simplify's
 * clustering grid has as well) */
const uint32_t CELL_BITS = 21;
const uint32_t CELL_CAP = 1u << CELL_BITS;
const uint32_t EXTENT_BITS = 20;                /* a triangle's extent as a fraction of the box's, in the classify sum */
const uint64_t MIN_RECORD_BUDGET = uint64_t(1) << 20;
const uint32_t RECORDS_PER_TRIANGLE = 8;        /* the budget: what the records may cost per triangle that takes part */

/* what the (cell, triangle) records of `live` triangles may number */
inline uint64_t recordBudget(uint64_t live) { return std::max(MIN_RECORD_BUDGET, (uint64_t) RECORDS_PER_TRIANGLE * live); }

/* a cell packed whatever the grid: z << 42 | y << 21 | x */
MLSGPU_HD inline uint64_t packCell(uint32_t x, uint32_t y, uint32_t z)
{
    return (uint64_t) z << (2 * CELL_BITS) | (uint64_t) y << CELL_BITS | x;
}

/* The sparse grid: cell (x, y, z) has the key z << (bx + by) | y << bx | x, the axes as wide as their cell counts need. */
struct Grid
{
    double origin[3];           /* the box's lower corner, lowered by reach */
    double h;
    uint32_t n[3];              /* cells per axis, each >= 1 and <= CELL_CAP */
    uint32_t shiftY, shiftZ;
    double reach;               /* how far a triangle's box is inflated: deviation's D; 0.0 for the self-intersection report */

    /* monotone in x: one subtraction, one division, floor, clamp (fmax and fmin hand back the bound for a NaN) */
    MLSGPU_HD inline uint32_t cell(int axis, double x) const
    {
        const double c = floor((x - origin[axis]) / h);
        return (uint32_t) fmin(fmax(c, 0.0), (double) (n[axis] - 1));
    }
    MLSGPU_HD inline uint64_t key(uint32_t x, uint32_t y, uint32_t z) const
    {
        return (uint64_t) z << shiftZ | (uint64_t) y << shiftY | x;
    }
    /* packCell() of the cell that has this key */
    MLSGPU_HD inline uint64_t packedOf(uint64_t key) const
    {
        const uint64_t x = key & ((uint64_t(1) << shiftY) - 1);
        const uint64_t y = (key >> shiftY) & ((uint64_t(1) << (shiftZ - shiftY)) - 1);
        return (key >> shiftZ) << (2 * CELL_BITS) | y << CELL_BITS | x;
    }
    MLSGPU_HD inline uint32_t keyBits() const { return shiftZ + bitLength(n[2] - 1); }
};

/* the grid of cell size h over [lo, hi] per axis, or false if an axis would need more than CELL_CAP cells (or h is a NaN) */
inline bool layGrid(const double lo[3], const double hi[3], double h, double reach, Grid *G)
{
    G->h = h;
    G->reach = reach;
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

/* The box of the finite vertex coordinates, inflated by reach, from the counter words the extent kernel leaves (per axis the
 * complement of the smallest and the largest, as ordered bits): no finite coordinate lies outside.  `side` is the longest
 * side before the inflation; a triangle's extent is summed in units of 2^-EXTENT_BITS of 2^eSide, the power of two above it.
 * Without vertices there is no triangle to bin, and the box is the origin. */
struct GridBox
{
    double lo[3], hi[3], side;
    int eSide;
};
inline GridBox boxOfWords(const unsigned long long *boxMin, const unsigned long long *boxMax, bool anyVertex, double reach)
{
    GridBox B = {{0, 0, 0}, {0, 0, 0}, 0.0, 0};
    if (anyVertex)
        for (int x = 0; x < 3; x++)
        {
            const double least = (double) fromOrdered(~(uint32_t) boxMin[x]), most = (double) fromOrdered((uint32_t) boxMax[x]);
            B.side = std::max(B.side, most - least);
            B.lo[x] = least - reach;
            B.hi[x] = most + reach;
        }
    uint64_t bitsOfSide;
    std::memcpy(&bitsOfSide, &B.side, sizeof(B.side));
    B.eSide = B.side > 0.0 ? exponentOfDoubleBits(bitsOfSide) + 1 : 0;
    return B;
}

/* The first cell: twice the reach, or the mean extent of a live triangle's box where that is larger; where neither is
 * positive (no reach, and every triangle a point) the box's longest side, or 1.  live > 0. */
inline double firstCellSize(uint64_t extentSum, uint64_t live, int eSide, double side, double reach)
{
    const double meanExtent = (double) extentSum / (double) live * powerOfTwo(eSide - (int) EXTENT_BITS);
    const double first = std::max(2.0 * reach, meanExtent);
    return first > 0.0 ? first : side > 0.0 ? side : 1.0;
}

} // namespace mlsgpu

#endif
