/*
 * Stand-alone driver of bucketplan.hpp for tests/test_bucket_plan.py (not part of libmlsgpu_hip.so): one case on stdin, what
 * the bucketer would decide for it on stdout.
 *
 * stdin:   dims[3] lo[3] n maxSplats maxCells maxSplit chunkCells microCells withCounts
 *          then, if withCounts is 1, for every chunk (x-major, as the bucketer visits them) its totalNodes counters
 * stdout:  plan    microSize chunkCells chunks[3] macroLevels chunkRatio ok
 *          chunk   cc[3] sub.lo[3] sub.hi[3] dims[3] bias[3] totalNodes n0 ok
 *          level   l dims[3] offset                (per level of the chunk)
 *          picked  ok numRegions                   (with counters)
 *          region  c[3] level count box.lo[3] box.hi[3]
 *          table   one word per microblock
 */
#include "bucketplan.hpp"

#include <cinttypes>
#include <cstdio>

using namespace mlsgpu;

static void print3(const uint32_t v[3]) { std::printf(" %" PRIu32 " %" PRIu32 " %" PRIu32, v[0], v[1], v[2]); }
static void print3(const int32_t v[3]) { std::printf(" %" PRId32 " %" PRId32 " %" PRId32, v[0], v[1], v[2]); }

int main()
{
    uint32_t dims[3], chunkCells, microCells;
    GridBox grid;
    uint64_t n;
    mlsgpu_bucket_params P = {};
    int withCounts = 0;
    if (std::scanf("%" SCNu32 "%" SCNu32 "%" SCNu32 "%" SCNd32 "%" SCNd32 "%" SCNd32 "%" SCNu64 "%" SCNu64 "%" SCNu32 "%" SCNu64
                   "%" SCNu32 "%" SCNu32 "%d", &dims[0], &dims[1], &dims[2], &grid.lo[0], &grid.lo[1], &grid.lo[2], &n, &P.maxSplats,
                   &P.maxCells, &P.maxSplit, &chunkCells, &microCells, &withCounts) != 13)
        return 2;
    for (int i = 0; i < 3; i++)
        grid.hi[i] = (int32_t) (grid.lo[i] + (int64_t) dims[i]);
    LevelPlan plan;
    const bool planned = planLevel(dims, n, P, chunkCells, microCells, &plan);
    std::printf("plan %" PRIu32 " %" PRIu32, plan.microSize, plan.chunkCells);
    print3(plan.chunks);
    std::printf(" %" PRIu32 " %" PRIu32 " %d\n", plan.macroLevels, plan.chunkRatio, (int) planned);
    if (!planned)
        return 0;
    for (uint32_t cx = 0; cx < plan.chunks[0]; cx++)
        for (uint32_t cy = 0; cy < plan.chunks[1]; cy++)
            for (uint32_t cz = 0; cz < plan.chunks[2]; cz++)
            {
                const uint32_t cc[3] = {cx, cy, cz};
                ChunkLayout C;
                const bool laid = layoutChunk(plan, grid, cc, &C);
                std::printf("chunk");
                print3(cc);
                print3(C.sub.lo);
                print3(C.sub.hi);
                print3(C.dims);
                print3(C.bias);
                std::printf(" %" PRIu64 " %" PRIu32 " %d\n", laid ? C.totalNodes : 0, laid ? C.n0 : 0, (int) laid);
                if (!laid)
                    continue;
                for (uint32_t l = 0; l < C.L.levels; l++)
                {
                    std::printf("level %" PRIu32, l);
                    print3(C.L.dims[l]);
                    std::printf(" %" PRIu32 "\n", C.L.offset[l]);
                }
                if (!withCounts)
                    continue;
                std::vector<uint32_t> counts(C.totalNodes);
                for (uint32_t &c : counts)
                    if (std::scanf("%" SCNu32, &c) != 1)
                        return 2;
                std::vector<Region> regions;
                std::vector<uint32_t> table;
                const bool picked = pickRegions(counts.data(), C.L, C.dims, plan.microSize, P.maxCells, P.maxSplats, &regions, &table);
                std::printf("picked %d %zu\n", (int) picked, regions.size());
                for (const Region &g : regions)
                {
                    const GridBox box = regionBox(g, plan.microSize, C.sub);
                    std::printf("region");
                    print3(g.c);
                    std::printf(" %" PRIu32 " %" PRIu32, g.level, g.count);
                    print3(box.lo);
                    print3(box.hi);
                    std::printf("\n");
                }
                std::printf("table");
                for (uint32_t t : table)
                    std::printf(" %" PRIu32, t);
                std::printf("\n");
            }
    return 0;
}
