/*
 * The host arithmetic of one bucketing level (bucket.hip): how a grid is cut into chunks and microblocks, how a chunk's
 * dense octree of counters is laid out, which nodes become regions, and a region's box.  Both routes of the bucketer --
 * a resident cloud and the streamed top level -- split a level by these functions.  Plain C++17, no HIP: a stand-alone
 * program (bucketplan_test.cpp) runs it without a GPU.
 */
#ifndef MLSGPU_BUCKETPLAN_HPP
#define MLSGPU_BUCKETPLAN_HPP

#include "../../include/mlsgpu_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace mlsgpu
{

enum { MAX_LEVELS = 32 };

struct GridBox
{
    int32_t lo[3], hi[3];
    uint32_t cells(int i) const { return (uint32_t) (hi[i] - lo[i]); }
};

/* a chunk's octree of microblock counters, finest level first (a kernel argument: the layout is fixed) */
struct LevelLayout
{
    uint32_t levels;
    uint32_t dims[MAX_LEVELS][3];
    uint32_t offset[MAX_LEVELS + 1];
};

inline uint64_t mulSat(uint64_t a, uint64_t b)
{
    if (a == 0 || b == 0)
        return 0;
    return a > UINT64_MAX / b ? UINT64_MAX : a * b;
}

/* microblocks of a grid of `dims` cells, saturating */
inline uint64_t microBlocksOf(const uint32_t dims[3], uint32_t microSize)
{
    uint64_t b = 1;
    for (int i = 0; i < 3; i++)
        b = mulSat(b, ((uint64_t) dims[i] + microSize - 1) / microSize);
    return b;
}

/* chooseMicroSize, src/bucket.cpp:354-377 */
inline uint32_t chooseMicroSize(const uint32_t dims[3], uint64_t maxSplit, uint64_t numSplats, uint64_t maxSplats, uint32_t maxCells)
{
    uint32_t microSize = 1;
    uint64_t microBlocks = microBlocksOf(dims, microSize);
    const double target = 0.5 * std::min(std::min(dims[0], dims[1]), dims[2]) * std::sqrt((double) maxSplats / (double) numSplats);
    while (microBlocks > maxSplit || (microBlocks > 8 && microSize < target * 0.5 && (uint64_t) microSize * 2 <= maxCells))
    {
        microSize *= 2;
        microBlocks = microBlocksOf(dims, microSize);
    }
    return microSize;
}

/* the geometry of one level of bucketRecurse (src/bucket_impl.h:439-560) */
struct LevelPlan
{
    uint32_t microSize;         /* cells per microblock side */
    uint32_t chunkCells;        /* cells per chunk side: a multiple of microSize */
    uint32_t chunks[3];
    uint32_t macroLevels;       /* octree levels over a chunk's microblocks */
    uint32_t chunkRatio;        /* microblocks per chunk side */
};

/* false: a chunk needs more than MAX_LEVELS octree levels */
inline bool planLevel(const uint32_t cellDims[3], uint64_t n, const mlsgpu_bucket_params &P, uint32_t chunkCells, uint32_t microCells,
                      LevelPlan *plan)
{
    const uint32_t maxCellDim = std::max(std::max(cellDims[0], cellDims[1]), cellDims[2]);
    uint32_t microSize = microCells;
    if (microSize == 0 || microSize > maxCellDim)
        microSize = chooseMicroSize(cellDims, P.maxSplit, n, P.maxSplats, P.maxCells);
    while (microBlocksOf(cellDims, microSize) > P.maxSplit)
        microSize *= 2;
    chunkCells = chunkCells == 0 ? maxCellDim : std::min(maxCellDim, chunkCells);
    uint64_t grain = microSize;
    if (chunkCells > P.maxCells && P.maxCells >= microSize)
        grain = (uint64_t) P.maxCells / microSize * microSize;
    chunkCells = (uint32_t) ((chunkCells + grain - 1) / grain * grain);
    plan->microSize = microSize;
    plan->chunkCells = chunkCells;
    for (int i = 0; i < 3; i++)
        plan->chunks[i] = (cellDims[i] + chunkCells - 1) / chunkCells;
    plan->macroLevels = 1;
    while (((uint64_t) microSize << (plan->macroLevels - 1)) < chunkCells)
        plan->macroLevels++;
    plan->chunkRatio = chunkCells / microSize;
    return plan->macroLevels <= MAX_LEVELS;
}

/* chunk cc of a level: its box (BucketStateSet, src/bucket.cpp:304-331), its microblocks and its octree of counters */
struct ChunkLayout
{
    GridBox sub;
    uint32_t dims[3];           /* microblocks */
    uint32_t bias[3];           /* the chunk's first microblock, counted from the grid's lower end */
    LevelLayout L;
    uint64_t totalNodes;
    uint32_t n0;                /* nodes of level 0: the microblocks */
};

/* false: more than 2^24 nodes (the counters are dense; the reference hashes) */
inline bool layoutChunk(const LevelPlan &plan, const GridBox &grid, const uint32_t cc[3], ChunkLayout *out)
{
    for (int i = 0; i < 3; i++)
    {
        const int64_t off = (int64_t) cc[i] * plan.chunkCells;
        out->sub.lo[i] = (int32_t) (grid.lo[i] + off);
        out->sub.hi[i] = (int32_t) std::min<int64_t>(grid.lo[i] + off + plan.chunkCells, grid.hi[i]);
        out->bias[i] = cc[i] * plan.chunkRatio;
        out->dims[i] = (out->sub.cells(i) + plan.microSize - 1) / plan.microSize;
    }
    LevelLayout &L = out->L;
    L.levels = plan.macroLevels;
    uint64_t totalNodes = 0;
    for (uint32_t l = 0; l < plan.macroLevels; l++)
    {
        L.offset[l] = (uint32_t) totalNodes;
        uint64_t t = 1;
        for (int i = 0; i < 3; i++)
        {
            L.dims[l][i] = (uint32_t) (((uint64_t) out->dims[i] + ((uint64_t) 1 << l) - 1) >> l);
            t *= L.dims[l][i];
        }
        totalNodes += t;
        if (totalNodes > (1u << 24))
            return false;
    }
    L.offset[plan.macroLevels] = (uint32_t) totalNodes;
    out->totalNodes = totalNodes;
    out->n0 = out->dims[0] * out->dims[1] * out->dims[2];
    return true;
}

/* an octree node chosen as a region: coordinates at its level, and its counter -- the splats that join it */
struct Region
{
    uint32_t c[3];
    uint32_t level;
    uint32_t count;
};

/* pickNodes (src/bucket.cpp:248-269, PickNodes :333-352): depth-first, child 0 first, children x fastest; a node becomes a
 * region when it is a microblock or within both limits.  table[microblock] = region id << 5 | node level (0 where no region
 * covers it: only a microblock without splats).  false: more than 2^27 regions. */
inline bool pickRegions(const uint32_t *counts, const LevelLayout &L, const uint32_t dims[3], uint32_t microSize, uint32_t maxCells,
                        uint64_t maxSplats, std::vector<Region> *regions, std::vector<uint32_t> *table)
{
    struct Frame { uint32_t c[3]; uint32_t level; };
    regions->clear();
    table->assign((size_t) dims[0] * dims[1] * dims[2], 0);
    std::vector<Frame> stack;
    stack.push_back(Frame{{0, 0, 0}, L.levels - 1});
    while (!stack.empty())
    {
        const Frame f = stack.back();
        stack.pop_back();
        const uint32_t count = counts[L.offset[f.level] + (f.c[2] * L.dims[f.level][1] + f.c[1]) * L.dims[f.level][0] + f.c[0]];
        if (count == 0)
            continue;
        if (f.level == 0 || (((uint64_t) microSize << f.level) <= maxCells && count <= maxSplats))
        {
            const uint32_t id = (uint32_t) regions->size();
            if (id >= (1u << 27))
                return false;
            regions->push_back(Region{{f.c[0], f.c[1], f.c[2]}, f.level, count});
            uint32_t end[3];
            for (int j = 0; j < 3; j++)
                end[j] = (uint32_t) std::min<uint64_t>(dims[j], ((uint64_t) f.c[j] + 1) << f.level);
            for (uint32_t z = f.c[2] << f.level; z < end[2]; z++)
                for (uint32_t y = f.c[1] << f.level; y < end[1]; y++)
                    for (uint32_t x = f.c[0] << f.level; x < end[0]; x++)
                        (*table)[((size_t) z * dims[1] + y) * dims[0] + x] = (id << 5) | f.level;
            continue;
        }
        for (int idx = 7; idx >= 0; idx--)     /* pushed in reverse so that child 0 is visited first */
        {
            const Frame ch{{f.c[0] * 2 + (idx & 1), f.c[1] * 2 + ((idx >> 1) & 1), f.c[2] * 2 + (uint32_t) (idx >> 2)}, f.level - 1};
            bool inside = true;
            for (int j = 0; j < 3; j++)
                if (((uint64_t) ch.c[j] << ch.level) >= dims[j])
                    inside = false;
            if (inside)
                stack.push_back(ch);
        }
    }
    return true;
}

/* a region's cells, clipped to its chunk (Node::toCells, src/bucket.cpp:113-122) */
inline GridBox regionBox(const Region &g, uint32_t microSize, const GridBox &sub)
{
    GridBox box;
    for (int i = 0; i < 3; i++)
    {
        const uint64_t lower = ((uint64_t) microSize * g.c[i]) << g.level;
        const uint64_t upper = lower + ((uint64_t) microSize << g.level);
        box.lo[i] = (int32_t) (sub.lo[i] + (int64_t) std::min<uint64_t>(lower, sub.cells(i)));
        box.hi[i] = (int32_t) (sub.lo[i] + (int64_t) std::min<uint64_t>(upper, sub.cells(i)));
    }
    return box;
}

} // namespace mlsgpu
#endif
