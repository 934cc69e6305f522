/*
 * Stand-alone driver of meshgridplan.hpp for tests/test_meshgrid_plan.py (not part of libmlsgpu_hip.so): questions on stdin,
 * one a line, and what the grid's plan would decide on stdout, one line each.  Every double goes in and comes out as the
 * integer of its 64 bits, every float as that of its 32, so that nothing is rounded on the way.
 *
 *   GRID = lo0 lo1 lo2 hi0 hi1 hi2 h reach      (doubles)
 *   lay GRID                  -> lay accepted n0 n1 n2 shiftY shiftZ keyBits     (zeros behind a 0)
 *   cell GRID axis count x .. -> cell c ..                                       (doubles x; the grid must be accepted)
 *   key GRID x y z            -> key key packed x' y' z'                         (packed = packedOf(key); x' y' z' its fields)
 *   first extentSum live eSide side reach       -> first cellSize
 *   box min0 min1 min2 max0 max1 max2 any reach -> box lo0 lo1 lo2 hi0 hi1 hi2 side eSide      (the counter words)
 *   ordered bits              -> ordered orderedBits back                        (back: the bits of fromOrdered(orderedBits))
 *   budget live               -> budget records
 */
#include "meshgridplan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mlsgpu;

static bool read32(uint32_t *v) { return std::scanf("%" SCNu32, v) == 1; }
static bool read64(uint64_t *v) { return std::scanf("%" SCNu64, v) == 1; }
static bool readDouble(double *d)
{
    uint64_t bits;
    if (!read64(&bits))
        return false;
    std::memcpy(d, &bits, sizeof(*d));
    return true;
}
static uint64_t bitsOf(double d)
{
    uint64_t bits;
    std::memcpy(&bits, &d, sizeof(bits));
    return bits;
}
static bool readGrid(Grid *G, bool *accepted)
{
    double v[8];
    for (double &d : v)
        if (!readDouble(&d))
            return false;
    std::memset(G, 0, sizeof(*G));
    *accepted = layGrid(v, v + 3, v[6], v[7], G);
    return true;
}

int main()
{
    char what[16];
    while (std::scanf("%15s", what) == 1)
    {
        Grid G;
        bool accepted;
        if (std::strcmp(what, "lay") == 0)
        {
            if (!readGrid(&G, &accepted))
                return 2;
            if (accepted)
                std::printf("lay 1 %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", G.n[0], G.n[1], G.n[2],
                            G.shiftY, G.shiftZ, G.keyBits());
            else
                std::printf("lay 0 0 0 0 0 0 0\n");
        }
        else if (std::strcmp(what, "cell") == 0)
        {
            uint32_t axis, count;
            if (!(readGrid(&G, &accepted) && accepted && read32(&axis) && axis < 3 && read32(&count)))
                return 2;
            std::vector<double> x(count);
            for (double &d : x)
                if (!readDouble(&d))
                    return 2;
            std::printf("cell");
            for (double d : x)
                std::printf(" %" PRIu32, G.cell((int) axis, d));
            std::printf("\n");
        }
        else if (std::strcmp(what, "key") == 0)
        {
            uint32_t c[3];
            if (!(readGrid(&G, &accepted) && accepted && read32(&c[0]) && read32(&c[1]) && read32(&c[2])))
                return 2;
            const uint64_t key = G.key(c[0], c[1], c[2]), packed = G.packedOf(key), M = (uint64_t(1) << CELL_BITS) - 1;
            if (packed != packCell(c[0], c[1], c[2]))
                return 3;
            std::printf("key %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", key, packed, packed & M,
                        (packed >> CELL_BITS) & M, packed >> (2 * CELL_BITS));
        }
        else if (std::strcmp(what, "first") == 0)
        {
            uint64_t extentSum, live;
            int eSide;
            double side, reach;
            if (!(read64(&extentSum) && read64(&live) && std::scanf("%d", &eSide) == 1 && readDouble(&side) && readDouble(&reach)))
                return 2;
            std::printf("first %" PRIu64 "\n", bitsOf(firstCellSize(extentSum, live, eSide, side, reach)));
        }
        else if (std::strcmp(what, "box") == 0)
        {
            uint64_t w[6];
            unsigned long long words[6];
            uint32_t any;
            double reach;
            for (int k = 0; k < 6; k++)
            {
                if (!read64(&w[k]))
                    return 2;
                words[k] = w[k];
            }
            if (!(read32(&any) && readDouble(&reach)))
                return 2;
            const GridBox B = boxOfWords(words, words + 3, any != 0, reach);
            std::printf("box");
            for (int x = 0; x < 3; x++)
                std::printf(" %" PRIu64, bitsOf(B.lo[x]));
            for (int x = 0; x < 3; x++)
                std::printf(" %" PRIu64, bitsOf(B.hi[x]));
            std::printf(" %" PRIu64 " %d\n", bitsOf(B.side), B.eSide);
        }
        else if (std::strcmp(what, "ordered") == 0)
        {
            uint32_t bits, back;
            if (!read32(&bits))
                return 2;
            const uint32_t o = orderedBits(bits);
            const float f = fromOrdered(o);
            std::memcpy(&back, &f, sizeof(back));
            std::printf("ordered %" PRIu32 " %" PRIu32 "\n", o, back);
        }
        else if (std::strcmp(what, "budget") == 0)
        {
            uint64_t live;
            if (!read64(&live))
                return 2;
            std::printf("budget %" PRIu64 "\n", recordBudget(live));
        }
        else
            return 2;
    }
    return 0;
}
