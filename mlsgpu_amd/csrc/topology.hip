/*
 * Topology report of an indexed triangle mesh that is resident in HBM: the "count-all" form of Manifold::isManifold
 * (test/manifold.h:98-232).  The reference stops at the first defect it meets; here every triangle and every vertex is
 * classified, the classes are counted, and the lowest index of each class is kept -- from which the reference's single
 * verdict follows (the lowest bad triangle if there is one, else the lowest classified vertex).  Every output is a count or a
 * minimum, so the report does not depend on the schedule.  DESIGN.md, "Topology report", has the memory formula.
 *
 *   init      per-vertex arrays and the counter block
 *   classify  one thread per triangle: its class, and three half-edge records (from, to) -> third vertex
 *   sort      the records by (from << b) | to, b = bit length of V: the outgoing half-edges of a vertex become one segment,
 *             ordered by their other end
 *   segments  one thread per record: where each vertex's segment starts and ends, repeated half-edges
 *   twins     one thread per record: is the opposite half-edge there (binary search in the other end's segment); unions
 *   links     one thread per vertex: the edges opposite the vertex must form one ring or disjoint runs
 *   roots     components and boundaries, counted only for a mesh that has no defect
 *
 * An index >= V is compared, counted and reported, never used as an address: the triangles of a record that reaches the
 * kernels behind classify have all three indices below V.
 */
#include "meshpost.hpp"
#include "unionfind.hpp"

using namespace mlsgpu;

namespace
{

/* the counter block, 64-bit words: what one device -> host copy brings back */
enum
{
    C_COUNT = 0,            /* [6] triangles / vertices per class, MLSGPU_TOPO_* */
    C_FIRST = 6,            /* [6] lowest index per class */
    C_DUPLICATE_EDGES = 12,
    C_BOUNDARY_EDGES = 13,
    C_COMPONENTS = 14,
    C_BOUNDARIES = 15,
    C_FAILED = 16,          /* the union-find's retry bound was reached (its low 32 bits are the flag) */
    C_WORDS = 17
};

const uint32_t NO_SEGMENT = 0xFFFFFFFFu;    /* 3 T < 2^32 - 1: never a record's index */

__global__ __launch_bounds__(256) void initKernel(uint64_t numVertices, uint32_t *segStart, uint32_t *compParent, uint32_t *bndParent,
                                                  uint8_t *duplicated, uint8_t *onBoundary, Counter *counters)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < C_WORDS)
        counters[i] = i >= C_FIRST && i < C_FIRST + 6 ? ~(Counter) 0 : 0;
    if (i < numVertices)
    {
        segStart[i] = NO_SEGMENT;
        compParent[i] = (uint32_t) i;
        bndParent[i] = (uint32_t) i;
        duplicated[i] = 0;
        onBoundary[i] = 0;
    }
}

/* a. The class of a triangle is the first check that fails in the reference's rotation order (test/manifold.h:117-132): not
 *    meshpost.hpp's defectOf, which looks at the range of all three indices first.  A bad triangle's three records are dead. */
__global__ __launch_bounds__(256) void classifyKernel(const uint32_t *tri, uint64_t numTriangles, SideKeys K, uint64_t *keys,
                                                      uint32_t *vals, Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint64_t numVertices = K.numVertices;
    const uint64_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    int cls = MLSGPU_TOPO_NONE;
    if (i0 >= numVertices) cls = MLSGPU_TOPO_OUT_OF_RANGE;
    else if (i0 == i1) cls = MLSGPU_TOPO_DEGENERATE;
    else if (i1 >= numVertices) cls = MLSGPU_TOPO_OUT_OF_RANGE;
    else if (i1 == i2) cls = MLSGPU_TOPO_DEGENERATE;
    else if (i2 >= numVertices) cls = MLSGPU_TOPO_OUT_OF_RANGE;
    else if (i2 == i0) cls = MLSGPU_TOPO_DEGENERATE;
    tally(cls == MLSGPU_TOPO_OUT_OF_RANGE, &counters[C_COUNT + MLSGPU_TOPO_OUT_OF_RANGE], t, &counters[C_FIRST + MLSGPU_TOPO_OUT_OF_RANGE]);
    tally(cls == MLSGPU_TOPO_DEGENERATE, &counters[C_COUNT + MLSGPU_TOPO_DEGENERATE], t, &counters[C_FIRST + MLSGPU_TOPO_DEGENERATE]);
    if (cls != MLSGPU_TOPO_NONE)
    {
        for (int k = 0; k < 3; k++)
        {
            keys[3 * t + k] = K.dead();
            vals[3 * t + k] = 0;
        }
        return;
    }
    keys[3 * t + 0] = K.keyOf(i0, i1); vals[3 * t + 0] = (uint32_t) i2;
    keys[3 * t + 1] = K.keyOf(i1, i2); vals[3 * t + 1] = (uint32_t) i0;
    keys[3 * t + 2] = K.keyOf(i2, i0); vals[3 * t + 2] = (uint32_t) i1;
}

/* c, first half: the vertices' segments in the sorted records (R.vals: the third vertex of the record's triangle).  The plain
 * byte stores race only with stores of the same value. */
__global__ __launch_bounds__(256) void segmentsKernel(Records R, uint32_t *segStart, uint32_t *segEnd, uint8_t *duplicated, Counter *counters)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n)
        return;
    const uint64_t key = R.keys[i], from = R.fromOf(key);
    if (from >= R.numVertices)
        return;                 /* a bad triangle's record */
    if (R.segmentStart(i, from))
        segStart[from] = (uint32_t) i;
    if (R.segmentEnd(i, from))
        segEnd[from] = (uint32_t) (i + 1);
    const bool repeat = !R.head(i, key);
    if (repeat)
    {
        duplicated[from] = 1;
        duplicated[R.toOf(key)] = 1;
    }
    tally(repeat, &counters[C_DUPLICATE_EDGES]);
}

/* c, second half: needs every segment, hence a launch of its own.  noTwin[i] = 1 if the half-edge opposite to record i is
 * absent.  The first record of each distinct half-edge unites its ends in the component forest, and -- if it has no twin --
 * counts as a boundary edge and unites its ends in the boundary forest. */
__global__ __launch_bounds__(256) void twinsKernel(Records R, const uint32_t *segStart, const uint32_t *segEnd, uint32_t *noTwin,
                                                   uint8_t *onBoundary, uint32_t *compParent, uint32_t *bndParent, Counter *counters)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R.n)
        return;
    const uint64_t key = R.keys[i], from = R.fromOf(key);
    if (from >= R.numVertices)
        return;
    const uint32_t to = R.toOf(key);
    const uint32_t lo = segStart[to];
    bool twin = false;
    if (lo != NO_SEGMENT)
    {
        const uint32_t hi = segEnd[to];
        twin = R.find(lo, hi, R.keyOf(to, from)) != hi;
    }
    noTwin[i] = twin ? 0u : 1u;
    const bool first = R.head(i, key);
    const bool boundary = first && !twin;
    tally(boundary, &counters[C_BOUNDARY_EDGES]);
    uint32_t *const failed = reinterpret_cast<uint32_t *>(&counters[C_FAILED]);
    if (boundary)
    {
        onBoundary[from] = 1;
        onBoundary[to] = 1;
        unite(bndParent, (uint32_t) from, to, failed, UNION_SHORTCUT);
    }
    if (first)
        unite(compParent, (uint32_t) from, to, failed, UNION_SHORTCUT);
}

/* d. The records of vertex v are (v -> x, y) for its triangles (v, x, y): arrow[x] = y, looked up by binary search in v's own
 *    segment.  A run starts at an x whose half-edge v -> x has no twin.  No x and no y repeats here (the vertex would be
 *    DUPLICATED), so the runs are disjoint paths and a ring closes; every walk is bounded by the degree all the same. */
__global__ __launch_bounds__(256) void linksKernel(Records R, const uint32_t *segStart, const uint32_t *segEnd, const uint32_t *noTwin,
                                                   const uint8_t *duplicated, Counter *counters)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= R.numVertices)
        return;
    const uint32_t s = segStart[v];
    int cls = MLSGPU_TOPO_NONE;
    if (s == NO_SEGMENT)
        cls = MLSGPU_TOPO_ISOLATED;
    else if (duplicated[v])
        cls = MLSGPU_TOPO_DUPLICATED;
    else
    {
        const uint32_t e = segEnd[v], deg = e - s;
        uint32_t length = 0;
        bool runs = false;
        for (uint32_t i = s; i < e; i++)
            if (noTwin[i])
            {
                runs = true;
                uint32_t cur = R.toOf(R.keys[i]);
                while (length <= deg)       /* beyond deg the verdict is MIXED already */
                {
                    const uint32_t at = R.find(s, e, R.keyOf(v, cur));
                    if (at == e)
                        break;
                    cur = R.vals[at];
                    length++;
                }
            }
        if (runs)
        {
            if (length != deg)
                cls = MLSGPU_TOPO_MIXED;
        }
        else
        {
            /* rings only: there must be exactly one, so the walk from any x is back after deg steps and not before */
            const uint32_t start = R.toOf(R.keys[s]);
            uint32_t cur = start, steps = 0;
            bool closed = false;
            while (steps < deg)
            {
                const uint32_t at = R.find(s, e, R.keyOf(v, cur));
                if (at == e)
                    break;
                cur = R.vals[at];
                steps++;
                if (cur == start)
                {
                    closed = true;
                    break;
                }
            }
            if (!closed || steps != deg)
                cls = MLSGPU_TOPO_TUNNEL;
        }
    }
#pragma unroll
    for (int k = MLSGPU_TOPO_ISOLATED; k <= MLSGPU_TOPO_TUNNEL; k++)
        tally(cls == k, &counters[C_COUNT + k], v, &counters[C_FIRST + k]);
}

/* e. Only for a mesh without defects (the counters of the kernels before are complete: a launch lies between).
 *    numBoundaries: the reference counts the sets of at least 3 vertices in a forest where every vertex is a set of its own
 *    and the two ends of each boundary edge are united (test/manifold.h:193-195, 223-227).  A set of exactly two vertices
 *    cannot exist -- it would take the two half-edges a -> b and b -> a, which are each other's twins and hence no boundary
 *    edges -- so the sets of 3 or more are exactly those of the vertices that touch a boundary edge, and counting the roots
 *    among those vertices gives the same number. */
__global__ __launch_bounds__(256) void rootsKernel(uint64_t numVertices, const uint32_t *compParent, const uint32_t *bndParent,
                                                   const uint8_t *onBoundary, Counter *counters)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    Counter defects = 0;
    for (int k = 0; k < 6; k++)
        defects |= counters[C_COUNT + k];
    if (defects != 0 || v >= numVertices)
        return;
    tally(compParent[v] == (uint32_t) v, &counters[C_COMPONENTS]);
    tally(onBoundary[v] != 0 && bndParent[v] == (uint32_t) v, &counters[C_BOUNDARIES]);
}

/* the verdict and what follows from the counts */
void conclude(mlsgpu_topology *t, uint64_t components, uint64_t boundaries)
{
    t->manifold = 1;
    for (int k = 0; k < 6; k++)
        if (t->count[k] != 0)
            t->manifold = 0;
    t->firstKind = MLSGPU_TOPO_NONE;
    t->firstIndex = UINT64_MAX;
    /* the reference meets every triangle before any vertex */
    const int groups[2][2] = {{MLSGPU_TOPO_OUT_OF_RANGE, MLSGPU_TOPO_DEGENERATE}, {MLSGPU_TOPO_ISOLATED, MLSGPU_TOPO_TUNNEL}};
    for (int g = 0; g < 2 && t->firstKind == MLSGPU_TOPO_NONE; g++)
        for (int k = groups[g][0]; k <= groups[g][1]; k++)
            if (t->firstOf[k] < t->firstIndex)
            {
                t->firstIndex = t->firstOf[k];
                t->firstKind = (uint32_t) k;
            }
    if (t->manifold)
    {
        t->edges = (3 * t->numTriangles + t->boundaryEdges) / 2;
        t->eulerCharacteristic = (int64_t) t->numVertices - (int64_t) t->edges + (int64_t) t->numTriangles;
        t->numComponents = components;
        t->numBoundaries = boundaries;
    }
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_topology(mlsgpu_ctx *ctx, const uint32_t *dTriangles, uint64_t numTriangles, uint64_t numVertices,
                                        mlsgpu_topology *out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    /* the sort's values and tile counts are 32-bit, and so are the indices of a triangle */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3, MLSGPU_ERR_LENGTH);
    REQUIRE(numTriangles == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    std::memset(out, 0, sizeof(*out));
    out->numVertices = numVertices;
    out->numTriangles = numTriangles;
    for (int k = 0; k < 6; k++)
        out->firstOf[k] = UINT64_MAX;
    if (numTriangles == 0)
    {
        /* every vertex is isolated; no vertices and no triangles is the reference's (manifold) empty mesh */
        out->count[MLSGPU_TOPO_ISOLATED] = numVertices;
        if (numVertices > 0)
            out->firstOf[MLSGPU_TOPO_ISOLATED] = 0;
        conclude(out, 0, 0);
        return MLSGPU_OK;
    }

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t n = 3 * numTriangles, nv = numVertices;
    const SideKeys K = SideKeys::of(nv);
    SortScratch sides;
    DeviceArray<uint32_t> segStart, segEnd, compParent, bndParent;
    DeviceArray<uint8_t> duplicated, onBoundary;
    DeviceArray<Counter> counters;
    PROPAGATE(sides.alloc(n));
    PROPAGATE(segStart.alloc(nv));
    PROPAGATE(segEnd.alloc(nv));
    PROPAGATE(compParent.alloc(nv));
    PROPAGATE(bndParent.alloc(nv));
    PROPAGATE(duplicated.alloc(nv));
    PROPAGATE(onBoundary.alloc(nv));
    PROPAGATE(counters.alloc(C_WORDS));
    if (ctx->timing)
        ctx->addValue("topology.scratch.bytes",
                      (double) (sides.bytes() + 4 * segStart.bytes(nv) + 2 * duplicated.bytes(nv) + counters.bytes(C_WORDS)));

    const dim3 B(256);
    LAUNCH(ctx, "kernel.topology.init", initKernel, dim3(divUp(std::max<uint64_t>(nv, C_WORDS), 256)), B, nv, segStart.get(),
           compParent.get(), bndParent.get(), duplicated.get(), onBoundary.get(), counters.get());
    LAUNCH(ctx, "kernel.topology.classify", classifyKernel, dim3(divUp(numTriangles, 256)), B, dTriangles, numTriangles, K,
           sides.keys(), sides.vals(), counters.get());
    Records R;
    PROPAGATE(sides.sort(ctx, "kernel.topology.sort", K, false, &R));
    uint32_t *const noTwin = sides.freeVals();          /* one word per record for the twins pass */
    if (nv > 0)
    {
        LAUNCH(ctx, "kernel.topology.segments", segmentsKernel, dim3(divUp(n, 256)), B, R, segStart.get(), segEnd.get(), duplicated.get(),
               counters.get());
        LAUNCH(ctx, "kernel.topology.twins", twinsKernel, dim3(divUp(n, 256)), B, R, (const uint32_t *) segStart.get(),
               (const uint32_t *) segEnd.get(), noTwin, onBoundary.get(), compParent.get(), bndParent.get(), counters.get());
        LAUNCH(ctx, "kernel.topology.links", linksKernel, dim3(divUp(nv, 256)), B, R, (const uint32_t *) segStart.get(),
               (const uint32_t *) segEnd.get(), (const uint32_t *) noTwin, (const uint8_t *) duplicated.get(), counters.get());
        LAUNCH(ctx, "kernel.topology.roots", rootsKernel, dim3(divUp(nv, 256)), B, nv, (const uint32_t *) compParent.get(),
               (const uint32_t *) bndParent.get(), (const uint8_t *) onBoundary.get(), counters.get());
    }
    Counter h[C_WORDS];
    HIP_CHECK(hipMemcpyAsync(h, counters.get(), sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h[C_FAILED] != 0)
        return setError(MLSGPU_ERR_HIP, "mesh topology: the union-find did not settle within its retry bound");
    for (int k = 0; k < 6; k++)
    {
        out->count[k] = h[C_COUNT + k];
        out->firstOf[k] = h[C_FIRST + k];
    }
    out->duplicateEdges = h[C_DUPLICATE_EDGES];
    out->boundaryEdges = h[C_BOUNDARY_EDGES];
    conclude(out, h[C_COMPONENTS], h[C_BOUNDARIES]);
    return MLSGPU_OK;
}

MLSGPU_API uint64_t mlsgpu_hip_topology_reason(const mlsgpu_topology *t, char *buf, uint64_t len)
{
    char text[96];
    text[0] = '\0';
    if (t != nullptr)
    {
        const unsigned long long i = t->firstIndex;
        switch (t->firstKind)
        {
        case MLSGPU_TOPO_OUT_OF_RANGE: snprintf(text, sizeof(text), "Triangle %llu contains an out-of-range index", i); break;
        case MLSGPU_TOPO_DEGENERATE: snprintf(text, sizeof(text), "Triangle %llu contains a vertex twice", i); break;
        case MLSGPU_TOPO_ISOLATED: snprintf(text, sizeof(text), "Vertex %llu is isolated", i); break;
        case MLSGPU_TOPO_DUPLICATED: snprintf(text, sizeof(text), "Vertex %llu is on an edge that occurs twice with same winding", i); break;
        case MLSGPU_TOPO_MIXED: snprintf(text, sizeof(text), "Vertex %llu is both in the interior and on the boundary", i); break;
        case MLSGPU_TOPO_TUNNEL: snprintf(text, sizeof(text), "Vertex %llu tunnels between interior regions", i); break;
        default: break;
        }
    }
    const uint64_t need = std::strlen(text);
    if (buf != nullptr && len > 0)
    {
        const uint64_t n = need < len - 1 ? need : len - 1;
        std::memcpy(buf, text, n);
        buf[n] = '\0';
    }
    return need;
}
