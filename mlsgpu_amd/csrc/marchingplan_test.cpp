/*
 * Stand-alone driver of marchingplan.hpp for tests/test_marching_plan.py (not part of libmlsgpu_hip.so): questions on
 * stdin, one a line, and what marching would decide on stdout, one line each.
 *
 *   sizes W H D swatheLimit meshMemory a0 a1 a2
 *       -> sizes imageWidth imageHeight zStride maxSwathe swatheCells vertexSpace indexSpace fieldRows legacyBuffers
 *                latRowsMax latWords
 *   lattice W H zTop zMax latRowsMax latWords
 *       -> lattice nw rowsPerLayer topx topy z2First z2Last cw ch numRows cornerRows cellRows numWords numQuads
 *                  maskGroups(rows) maskGroups(words; 0 if nw > 64) fits
 *   mask nw forced                                  -> mask 0|1
 *   triangles nw occupied cellRows cw forced        -> triangles 0|1           (forced: -1, 0 or 1)
 *   weld depth maxSwathe legacyBuffers forceSort    -> weld 0|1|2              (lattice, sort, none)
 *   keys W H D                                      -> keys bx by bz bits wideKeys
 *   run first last offsets0 offsets1 vertexSpace indexSpace n v0 i0 v1 i1 ...   (n slices, hist[0] first)
 *       -> run end
 */
#include "marchingplan.hpp"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace mlsgpu;

static bool read32(uint32_t *v) { return std::scanf("%" SCNu32, v) == 1; }
static bool read64(uint64_t *v) { return std::scanf("%" SCNu64, v) == 1; }

int main()
{
    char what[16];
    while (std::scanf("%15s", what) == 1)
    {
        if (std::strcmp(what, "sizes") == 0)
        {
            uint32_t v[4], a[3];
            uint64_t mem;
            if (!(read32(&v[0]) && read32(&v[1]) && read32(&v[2]) && read32(&v[3]) && read64(&mem) && read32(&a[0]) && read32(&a[1])
                  && read32(&a[2])))
                return 2;
            const MarchingSizes S(v[0], v[1], v[2], v[3], mem, a);
            std::printf("sizes %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
                        " %d %" PRIu64 " %" PRIu32 "\n", S.imageWidth, S.imageHeight, S.zStride, S.maxSwathe, S.swatheCells,
                        S.vertexSpace, S.indexSpace, S.fieldRows, (int) S.legacyBuffers, S.latRowsMax, S.latWords);
        }
        else if (std::strcmp(what, "lattice") == 0)
        {
            uint32_t v[4], latWords;
            uint64_t latRowsMax;
            if (!(read32(&v[0]) && read32(&v[1]) && read32(&v[2]) && read32(&v[3]) && read64(&latRowsMax) && read32(&latWords)))
                return 2;
            const LatticeDims D(v[0], v[1], v[2], v[3]);
            std::printf("lattice");
            for (uint32_t x : {D.nw, D.rowsPerLayer, D.topx, D.topy, D.z2First, D.z2Last, D.cw, D.ch, D.numRows, D.cornerRows,
                               D.cellRows, D.numWords(), D.numQuads(), D.maskGroups(true), D.nw <= 64 ? D.maskGroups(false) : 0u})
                std::printf(" %" PRIu32, x);
            std::printf(" %d\n", (int) D.fits(latRowsMax, latWords));
        }
        else if (std::strcmp(what, "mask") == 0)
        {
            uint32_t nw, forced;
            if (!(read32(&nw) && read32(&forced)))
                return 2;
            std::printf("mask %d\n", (int) maskByRows(nw, forced != 0));
        }
        else if (std::strcmp(what, "triangles") == 0)
        {
            uint32_t v[4];
            int forced;
            if (!(read32(&v[0]) && read32(&v[1]) && read32(&v[2]) && read32(&v[3]) && std::scanf("%d", &forced) == 1))
                return 2;
            std::printf("triangles %d\n", (int) trianglesByCells(v[0], v[1], v[2], v[3], forced));
        }
        else if (std::strcmp(what, "weld") == 0)
        {
            uint32_t v[4];
            if (!(read32(&v[0]) && read32(&v[1]) && read32(&v[2]) && read32(&v[3])))
                return 2;
            std::printf("weld %d\n", (int) weldRoute(v[0], v[1], v[2] != 0, v[3] != 0));
        }
        else if (std::strcmp(what, "keys") == 0)
        {
            uint32_t size[3];
            if (!(read32(&size[0]) && read32(&size[1]) && read32(&size[2])))
                return 2;
            const KeyBits k = keyLayout(size);
            std::printf("keys %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %d\n", k.bx, k.by, k.bz, k.bits(), (int) k.wideKeys());
        }
        else if (std::strcmp(what, "run") == 0)
        {
            uint32_t first, last, offsets[2], n;
            uint64_t space[2];
            if (!(read32(&first) && read32(&last) && read32(&offsets[0]) && read32(&offsets[1]) && read64(&space[0])
                  && read64(&space[1]) && read32(&n)))
                return 2;
            /* exactly n entries, so that a look behind `last` is the address sanitizer's to report */
            std::vector<SliceCounts> hist(n);
            for (SliceCounts &h : hist)
                if (!(read32(&h.vertices) && read32(&h.indices)))
                    return 2;
            std::printf("run %" PRIu32 "\n", sliceRun(hist.data(), first, last, offsets, space[0], space[1]));
        }
        else
            return 2;
    }
    return 0;
}
