/*
 * Part of marching.hip (its only includer): the lookup tables of marching tetrahedra as the reference builds them
 * (Marching::makeTables, src/marching.cpp:50-252) and what the kernels read instead of them -- the per-code records of the
 * lattice weld, the packed key table of the sort weld, the edge tables of the two mask kernels.  All host code but
 * DevTables, the device's view of the uploaded tables.
 */
#ifndef MLSGPU_MARCHING_TABLES_HPP
#define MLSGPU_MARCHING_TABLES_HPP

#include "common.hpp"
#include "marchingplan.hpp"

#include <algorithm>
#include <vector>

using namespace mlsgpu;

namespace
{

enum
{
    NUM_EDGES = 19,
    NUM_TETRAHEDRA = 6,
    NUM_CUBES = 256,
    KEY_AXIS_BITS = 21          /* (MAX_CELL_VERTICES and MAX_CELL_INDICES: marchingplan.hpp) */
};
const uint64_t KEY_EXTERNAL_FLAG = uint64_t(1) << 63;

/* src/marching.cpp:50-81 */
const unsigned char edgeIndices[NUM_EDGES][2] =
{
    {0, 1}, {0, 2}, {0, 3}, {1, 3}, {2, 3}, {0, 4}, {0, 5}, {1, 5}, {4, 5}, {0, 6},
    {2, 6}, {4, 6}, {0, 7}, {1, 7}, {2, 7}, {3, 7}, {4, 7}, {5, 7}, {6, 7}
};
const unsigned char tetrahedronIndices[NUM_TETRAHEDRA][4] =
{
    {0, 7, 1, 3}, {0, 7, 3, 2}, {0, 7, 2, 6}, {0, 7, 6, 4}, {0, 7, 4, 5}, {0, 7, 5, 1}
};

struct HostTables
{
    uint8_t count[NUM_CUBES][2];
    uint16_t start[NUM_CUBES + 1][2];
    std::vector<uint8_t> data;      /* vertex edge ids, then index lists */
    std::vector<uint32_t> key;      /* 3 per vertex entry */
};

unsigned int findEdge(unsigned int v0, unsigned int v1)
{
    if (v0 > v1) std::swap(v0, v1);
    for (unsigned int i = 0; i < NUM_EDGES; i++)
        if (edgeIndices[i][0] == v0 && edgeIndices[i][1] == v1)
            return i;
    return ~0u;
}

struct TetVertex
{
    unsigned char id;
    bool outside;
    bool operator<(const TetVertex &o) const { return id != o.id ? id < o.id : outside < o.outside; }
    bool operator>(const TetVertex &o) const { return o < *this; }
};

unsigned int parity4(const TetVertex *v)
{
    unsigned int p = 0;
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++)
            if (v[i] > v[j])
                p ^= 1;
    return p;
}

/* Marching::makeTables, src/marching.cpp:109-252: per cube code, walk the six tetrahedra around
 * diagonal 0-7; canonicalise each to "outside vertices first" by the first even permutation (w.r.t.
 * the tetrahedron's own orientation) that std::next_permutation yields, and emit 0, 1 or 2 triangles. */
void makeTables(HostTables &t)
{
    std::vector<uint8_t> vertexTable, indexTable;
    for (unsigned int cube = 0; cube < NUM_CUBES; cube++)
    {
        t.start[cube][0] = (uint16_t) vertexTable.size();
        t.start[cube][1] = (uint16_t) indexTable.size();
        std::vector<uint8_t> tri;
        for (unsigned int j = 0; j < NUM_TETRAHEDRA; j++)
        {
            TetVertex tv[4];
            unsigned int outside = 0;
            for (int k = 0; k < 4; k++)
            {
                tv[k].id = tetrahedronIndices[j][k];
                tv[k].outside = (cube >> tv[k].id) & 1;
                outside += tv[k].outside;
            }
            unsigned int baseParity = parity4(tv);
            if (outside > 2)
            {
                baseParity ^= 1;
                for (int k = 0; k < 4; k++)
                    tv[k].outside = !tv[k].outside;
            }
            std::sort(tv, tv + 4);
            do
            {
                if (parity4(tv) != baseParity)
                    continue;
                unsigned int mask = 0;
                for (int k = 0; k < 4; k++)
                    mask |= (unsigned int) tv[k].outside << k;
                const unsigned int t0 = tv[0].id, t1 = tv[1].id, t2 = tv[2].id, t3 = tv[3].id;
                if (mask == 0)
                    break;
                if (mask == 1)
                {
                    tri.push_back(findEdge(t0, t1)); tri.push_back(findEdge(t0, t3)); tri.push_back(findEdge(t0, t2));
                    break;
                }
                if (mask == 3)
                {
                    tri.push_back(findEdge(t0, t2)); tri.push_back(findEdge(t1, t2)); tri.push_back(findEdge(t1, t3));
                    tri.push_back(findEdge(t1, t3)); tri.push_back(findEdge(t0, t3)); tri.push_back(findEdge(t0, t2));
                    break;
                }
            } while (std::next_permutation(tv, tv + 4));
        }
        int compact[NUM_EDGES];
        int pool = 0;
        for (unsigned int e = 0; e < NUM_EDGES; e++)
            if (std::count(tri.begin(), tri.end(), (uint8_t) e))
            {
                compact[e] = pool++;
                vertexTable.push_back((uint8_t) e);
                for (int axis = 0; axis < 3; axis++)
                    t.key.push_back(((edgeIndices[e][0] >> axis) & 1) + ((edgeIndices[e][1] >> axis) & 1));
            }
        for (size_t k = 0; k < tri.size(); k++)
            indexTable.push_back((uint8_t) compact[tri[k]]);
        t.count[cube][0] = (uint8_t) (vertexTable.size() - t.start[cube][0]);
        t.count[cube][1] = (uint8_t) (indexTable.size() - t.start[cube][1]);
    }
    t.start[NUM_CUBES][0] = (uint16_t) vertexTable.size();
    t.start[NUM_CUBES][1] = (uint16_t) indexTable.size();
    for (unsigned int i = 0; i <= NUM_CUBES; i++)
        t.start[i][1] = (uint16_t) (t.start[i][1] + vertexTable.size());
    t.data = vertexTable;
    t.data.insert(t.data.end(), indexTable.begin(), indexTable.end());
}

/* latticeMaskKernel's table.  A corner (x, y, z) owns the lattice points towards +x, +y, +z, +xy, +xz, +yz, +xyz; the point on
 * an edge exists iff an occupied cell containing the edge sees different signs at its ends.  The cells are the eight around
 * the corner, (x - ox, y - dy, z - dz), in which the corner is local corner a = ox | dy << 1 | dz << 2.  Byte dy | dz << 1 of an
 * entry: what the cell gives as the corner's own cell (ox = 0); byte 4 + (dy | dz << 1): as the cell to its left (ox = 1),
 * which only holds the edges without an x component.  Bits: 0 +x, 1 +xy, 2 +xz, 3 +xyz, 5 +y, 6 +z, 7 +yz. */
std::vector<uint64_t> makeEdgeLut()
{
    std::vector<uint64_t> lut(256, 0);
    const int dir[7] = {1, 3, 5, 7, 2, 4, 6};          /* the edge's direction as a corner offset: +x, +xy, +xz, +xyz, +y, +z, +yz */
    const int bit[7] = {0, 1, 2, 3, 5, 6, 7};
    for (uint32_t code = 1; code < 255; code++)
        for (int ox = 0; ox < 2; ox++)
            for (int dy = 0; dy < 2; dy++)
                for (int dz = 0; dz < 2; dz++)
                {
                    const int a = ox | (dy << 1) | (dz << 2);
                    uint32_t bits = 0;
                    for (int e = 0; e < 7; e++)
                        if ((a & dir[e]) == 0)          /* the other end, a + dir, is a corner of the same cell */
                            bits |= (((code >> a) ^ (code >> (a | dir[e]))) & 1u) << bit[e];
                    lut[code] |= (uint64_t) bits << (8 * ((dy | (dz << 1)) + 4 * ox));
                }
    return lut;
}

/* latticeMaskWordKernel's tables, [r = dy | dz << 1][code]: low byte = what the cell gives the corner as its own cell, high
 * byte = as the cell to its left; bit 2h + 1 = the odd point of lattice row h (+x, +xy, +xz, +xyz), bit 2h = its even point
 * (h = 1 .. 3: +y, +z, +yz) -- a rearrangement of makeEdgeLut's bytes */
std::vector<uint16_t> makeEdgeLut16()
{
    const std::vector<uint64_t> lut = makeEdgeLut();
    auto remap = [](uint32_t old)
    {
        uint32_t v = 0;
        for (int h = 0; h < 4; h++)
        {
            v |= ((old >> h) & 1u) << (2 * h + 1);
            if (h > 0)
                v |= ((old >> (4 + h)) & 1u) << (2 * h);
        }
        return v;
    };
    std::vector<uint16_t> out(4 * 256, 0);
    for (uint32_t code = 0; code < 256; code++)
        for (int r = 0; r < 4; r++)
        {
            const uint32_t own = (uint32_t) (lut[code] >> (8 * r)) & 0xFFu, left = (uint32_t) (lut[code] >> (32 + 8 * r)) & 0xFFu;
            out[r * 256 + code] = (uint16_t) (remap(own) | remap(left) << 8);
        }
    return out;
}

/* the sort weld's key table: a vertex entry's three offsets in one word, kx | ky << 8 | kz << 16 */
std::vector<uint32_t> makePackedKeys(const HostTables &t)
{
    std::vector<uint32_t> packed(t.key.size() / 3);
    for (size_t i = 0; i < packed.size(); i++)
        packed[i] = t.key[3 * i] | (t.key[3 * i + 1] << 8) | (t.key[3 * i + 2] << 16);
    return packed;
}

/* the lattice weld's records, 16 words per cube code: DevTables::rec says what they hold */
std::vector<uint32_t> makeCodeRecords(const HostTables &t)
{
    std::vector<uint32_t> codeRec(NUM_CUBES * 16, 0u);
    for (uint32_t c = 0; c < NUM_CUBES; c++)
    {
        const uint32_t sv = t.start[c][0], si = t.start[c][1];
        const uint32_t nv = t.count[c][0], ni = t.count[c][1];
        uint64_t klo = 0;
        uint32_t khi = 0;
        for (uint32_t i = 0; i < nv; i++)
        {
            const uint32_t *k3 = &t.key[3 * (sv + i)];
            const uint64_t k6 = k3[0] | (k3[1] << 2) | (k3[2] << 4);
            if (i < 10) klo |= k6 << (6 * i); else khi |= (uint32_t) k6 << (6 * (i - 10));
        }
        uint32_t *rec = &codeRec[c * 16];
        rec[0] = (uint32_t) klo; rec[1] = (uint32_t) (klo >> 32); rec[2] = khi; rec[3] = nv | (ni << 8);
        for (uint32_t i = 0; i < ni; i++)
            rec[4 + i / 4] |= (uint32_t) t.data[si + i] << (8 * (i % 4));
        rec[13] = (ni & 3u) != 0 ? rec[4 + ni / 4] : 0u;
        if (nv != 0)
            for (uint32_t e = 0; e < NUM_EDGES; e++)
                rec[14] |= ((c >> edgeIndices[e][0] ^ c >> edgeIndices[e][1]) & 1u) << e;
        rec[15] = rec[3];
    }
    return codeRec;
}

/* ------------------------------------------------------------------ device side */

struct DevTables
{
    const uchar2 *count;     /* [256]  (vertices, indices) */
    const ushort2 *start;    /* [257] */
    const uint8_t *data;     /* [8192] */
    const uint32_t *key;     /* [2432] kx | ky<<8 | kz<<16 */
    const uint32_t *rec;     /* [256][16] per-code record for the lattice weld: words 0-1 = 6-bit keys (kx | ky<<2 | kz<<4) of
                              * vertices 0..9, word 2 = vertices 10..12, word 3 = nv | ni << 8, words 4..12 = index bytes,
                              * word 13 = the index word that is only partly used (0 if ni % 4 == 0), word 14 = the edges
                              * that carry a vertex (bit e), word 15 = word 3 again (so that words 4..15 are all the
                              * triangle emission reads) */
};

} // namespace

#endif
