/*
 * Vertex-clustering simplification of an indexed triangle mesh that is resident in HBM.  The reference has no counterpart:
 * its meshes leave the device whole (src/mesher.cpp:763-852).  The contract (include/mlsgpu_hip.h, DESIGN.md "Mesh
 * simplification") is written so that every output is an integer or one correctly rounded operation away from integers: the
 * result does not depend on the schedule.
 *
 *   bounds     a thread per vertex: its cell per axis (f32), validity, the largest cell per axis     } one read-back: errors,
 *   indices    a thread per index: indices >= V are counted                                         } bits of the cell key
 *   keys       a thread per vertex: the cell key, packed into as many bits as the largest cells need
 *   sort       (key, vertex id) by key: a cluster becomes a run
 *   clusters   a scan over the run heads: the cluster of every vertex and of every sorted position, where each run starts
 *   sums       a thread per sorted position: 2^-30 fixed-point offsets inside the cell, added up per cluster in 64-bit integers
 *              (a wave that lies inside one cluster adds once, a cluster of one member adds nothing)
 *   map        a thread per triangle: its three clusters, collapsed or rotated so that the smallest comes first
 *   survivors  a scan that packs the surviving triangles: (third cluster, triangle id)
 *   sort       stable by the third cluster, then (pairs kernel) stable by first << b | second: (first, second, third) order
 *   unique     a scan over "differs from its predecessor": the kept triangles, as cluster triples, and the clusters they use
 *   vertices   a scan over the used clusters: the dense numbering, and the position of every used cluster
 *   reindex    a thread per output index: cluster -> output vertex
 *
 * Quadric placement (mlsgpu_hip_mesh_simplify_quadric, steps 3a-3h of its contract) is the same run with other positions: the
 * cells, clusters, triangles and numbering above stay, and three pieces join them.
 *   extent     a thread per triangle, before the read-back: the face vector n in cell coordinates, the largest |component|
 *              (a 64-bit atomicMax on the bits of the double, at most one per wave and only where the wave's is larger than
 *              what the word holds); the host turns it into the shift of the fixed point
 *   quadrics   a thread per triangle, behind the clusters: n again, and per distinct cluster among its corners the six
 *              products n n^T and the three d n as 64-bit integers, added to the cluster's nine sums -- runs of one cluster
 *              among the lanes of a wave add up by shuffles first (MLSGPU_HIP_SIMPLIFY_ACCUMULATE=plain: every lane for itself)
 *   vertices   QuadricOut in VertexOut's place: the 3 x 3 solve per used cluster of several members, VertexOut's mean where
 *              it falls back
 *
 * An index >= V is compared and counted, never used as an address.
 *
 * Scratch belongs to the call: 60 bytes per vertex (the sort's two sides 24, cluster of a vertex 4, run starts 4, sums 24,
 * used / new index 4) and 44 bytes per triangle (cluster triple 12, the two sides of the 32-bit sort 16 and of the 64-bit
 * sort's keys 16), the sort's histogram (4 KB per 4096 elements of the larger of the two) and the scans' tile sums.  Quadric
 * placement takes 72 bytes per vertex more (nine sums per possible cluster, behind the mean's three) and four more counters.
 */
#include "meshpost.hpp"

#include <cmath>
#include <cstdlib>

using namespace mlsgpu;

namespace
{

/* 64-bit counters, read back twice */
enum
{
    C_BAD_VERTICES = 0,
    C_BAD_INDICES = 1,
    C_COLLAPSED = 2,
    C_WORDS = 3,
    /* quadric placement only */
    C_MAX_BITS = 3,             /* the bits of the largest |component| of a face vector, a double */
    C_SOLVED = 4,
    C_FLAT = 5,
    C_ESCAPED = 6,
    C_QUADRIC_WORDS = 7
};
/* 32-bit words: the largest cell per axis, and the totals the scans leave */
enum
{
    W_MAX_CELL = 0,     /* [3] */
    W_CLUSTERS = 3,
    W_SURVIVORS = 4,
    W_OUT_TRIANGLES = 5,
    W_OUT_VERTICES = 6,
    W_WORDS = 7
};

const uint32_t DROPPED = 0xFFFFFFFFu;       /* first cluster of a triangle that takes no further part; clusters are < V < 2^32 - 1 */
const float CELL_LIMIT = 2097152.0f;        /* 2^21 */
const double FIXED_ONE = 1073741824.0;      /* 2^30 */
const uint32_t NO_CLUSTER = 0xFFFFFFFFu;    /* what a lane that adds nothing holds: clusters are < V < 2^32 - 1 */
const int QUADRIC_SUMS = 9;                 /* A00 A01 A02 A11 A12 A22 b0 b1 b2 */

enum Placement
{
    PLACE_MEAN,
    PLACE_QUADRIC
};

struct Frame
{
    float origin[3];
    float cellSize;
};

/* how the three cells share a key: x in the low bits */
struct KeyBits
{
    uint32_t x, y, z;
    __host__ __device__ __forceinline__ uint64_t pack(const uint32_t c[3]) const
    {
        return (uint64_t) c[2] << (x + y) | (uint64_t) c[1] << x | c[0];
    }
    __device__ __forceinline__ void unpack(uint64_t key, uint32_t c[3]) const
    {
        c[0] = (uint32_t) (key & ((uint64_t(1) << x) - 1));
        c[1] = (uint32_t) ((key >> x) & ((uint64_t(1) << y) - 1));
        c[2] = (uint32_t) (key >> (x + y));
    }
};

/* step 1 of the contract: c = floorf((p - origin) / cellSize) per axis, two correctly rounded f32 operations; false for a
 * non-finite coordinate or a cell outside [0, 2^21) */
__device__ __forceinline__ bool cellOf(const float p[3], const Frame &F, uint32_t c[3])
{
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const float f = floorf((p[k] - F.origin[k]) / F.cellSize);
        const bool in = isfinite(p[k]) && f >= 0.0f && f < CELL_LIMIT;
        c[k] = in ? (uint32_t) f : 0u;
        ok = ok && in;
    }
    return ok;
}

/* Every lane of every wave stays to the end: waveMax needs the full wave. */
__global__ __launch_bounds__(256) void boundsKernel(const float *vertices, uint64_t numVertices, Frame F, Counter *counters, uint32_t *words)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = v < numVertices;
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (live)
    {
        p[0] = vertices[3 * v];
        p[1] = vertices[3 * v + 1];
        p[2] = vertices[3 * v + 2];
    }
    uint32_t c[3] = {0, 0, 0};
    const bool ok = !live || cellOf(p, F, c);
    tally(!ok, &counters[C_BAD_VERTICES]);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const uint32_t most = waveMax(live && ok ? c[k] : 0u);
        if (laneId() == 0 && most != 0)
            atomicMax(&words[W_MAX_CELL + k], most);
    }
}

__global__ __launch_bounds__(256) void indicesKernel(const uint32_t *indices, uint64_t numIndices, uint64_t numVertices, Counter *counters)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    tally(i < numIndices && indices[i] >= numVertices, &counters[C_BAD_INDICES]);
}

__global__ __launch_bounds__(256) void keysKernel(const float *vertices, uint64_t numVertices, Frame F, KeyBits bits, uint64_t *keys)
{
    const uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= numVertices)
        return;
    const float p[3] = {vertices[3 * v], vertices[3 * v + 1], vertices[3 * v + 2]};
    uint32_t c[3];
    cellOf(p, F, c);            /* every vertex is valid: the read-back behind boundsKernel said so */
    keys[v] = bits.pack(c);
}

/* ---- clusters: a scan over the heads of the sorted keys' runs ---- */
struct HeadIn
{
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return i == 0 || keys[i] != keys[i - 1] ? 1u : 0u; }
};
struct ClusterOut
{
    const uint32_t *sortedVertex;
    uint32_t *clusterOfVertex, *clusterOfPosition, *start;
    uint64_t numVertices;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t before, uint32_t head) const
    {
        const uint32_t cluster = before + head - 1;
        clusterOfVertex[sortedVertex[i]] = cluster;
        clusterOfPosition[i] = cluster;
        if (head)
            start[cluster] = (uint32_t) i;
        if (i + 1 == numVertices)
            start[cluster + 1] = (uint32_t) numVertices;
    }
};

/* step 3 of the contract, first half: q = llrint(((p - origin) / cellSize - c) * 2^30) in doubles, per axis */
__device__ __forceinline__ void fixedOffsets(const float p[3], const uint32_t c[3], const Frame &F, long long q[3])
{
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const double d = (double) p[k] - (double) F.origin[k];
        const double f = d / (double) F.cellSize - (double) c[k];
        q[k] = (long long) rint(f * FIXED_ONE);
    }
}

/* A thread per SORTED position, so that the members of a cluster are neighbours: a wave whose positions all lie in one
 * cluster (every wave but two of a large cluster) adds up in registers and issues three atomics; a cluster of one member
 * keeps its vertex and adds nothing.  No lane leaves early: the shuffles read every lane. */
__global__ __launch_bounds__(256) void sumsKernel(const float *vertices, const uint64_t *sortedKeys, const uint32_t *sortedVertex,
                                                  const uint32_t *clusterOfPosition, uint64_t numVertices, Frame F, KeyBits bits,
                                                  Counter *sums)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < numVertices;
    uint64_t key = 0, before = 0, after = 0;
    uint32_t v = 0, cluster = 0;
    if (live)
    {
        key = sortedKeys[i];
        before = i > 0 ? sortedKeys[i - 1] : ~key;
        after = i + 1 < numVertices ? sortedKeys[i + 1] : ~key;
        v = sortedVertex[i];
        cluster = clusterOfPosition[i];
    }
    const bool adds = live && (before == key || after == key);
    long long q[3] = {0, 0, 0};
    if (adds)
    {
        const float p[3] = {vertices[3 * (uint64_t) v], vertices[3 * (uint64_t) v + 1], vertices[3 * (uint64_t) v + 2]};
        uint32_t c[3];
        bits.unpack(key, c);
        fixedOffsets(p, c, F, q);
    }
    const uint64_t adders = __ballot(adds);
    if (adders == 0)
        return;                 /* (wave-uniform) */
    const uint32_t firstCluster = readLane(cluster, (int) __builtin_ctzll(adders));
    const bool oneCluster = __ballot(adds && cluster != firstCluster) == 0;
    if (oneCluster)
    {
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            const long long s = waveSum64(q[k]);        /* zero in the lanes that do not add */
            if (laneId() == 0)
                atomicAdd(&sums[3 * (uint64_t) firstCluster + k], (Counter) s);
        }
    }
    else if (adds)
    {
#pragma unroll
        for (int k = 0; k < 3; k++)
            atomicAdd(&sums[3 * (uint64_t) cluster + k], (Counter) q[k]);
    }
}

/* step 4, first half.  A triangle that collapses (or names a vertex that does not exist: counted before, never followed)
 * gets DROPPED as its first cluster. */
__global__ __launch_bounds__(256) void mapKernel(const uint32_t *triangles, uint64_t numTriangles, uint64_t numVertices,
                                                 const uint32_t *clusterOfVertex, uint32_t *mapped, Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= numTriangles)
        return;
    const uint32_t i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
    const bool inRange = i0 < numVertices && i1 < numVertices && i2 < numVertices;
    uint32_t a = DROPPED, b = 0, c = 0;
    bool collapsed = false;
    if (inRange)
    {
        a = clusterOfVertex[i0];
        b = clusterOfVertex[i1];
        c = clusterOfVertex[i2];
        collapsed = a == b || b == c || c == a;
        if (collapsed)
            a = DROPPED;
        else if (b < a && b < c)
        {
            const uint32_t x = a;
            a = b; b = c; c = x;
        }
        else if (c < a && c < b)
        {
            const uint32_t x = a;
            a = c; c = b; b = x;
        }
    }
    tally(collapsed, &counters[C_COLLAPSED]);
    mapped[3 * t] = a;
    mapped[3 * t + 1] = b;
    mapped[3 * t + 2] = c;
}

struct SurvivorIn
{
    const uint32_t *mapped;
    __device__ __forceinline__ uint32_t operator()(uint64_t t) const { return mapped[3 * t] != DROPPED ? 1u : 0u; }
};
struct SurvivorOut
{
    const uint32_t *mapped;
    uint32_t *third, *id;
    __device__ __forceinline__ void operator()(uint64_t t, uint32_t before, uint32_t survives) const
    {
        if (survives)
        {
            third[before] = mapped[3 * t + 2];
            id[before] = (uint32_t) t;
        }
    }
};

/* between the two sorts: the survivors in the order of their third cluster get first << b | second as their key */
__global__ __launch_bounds__(256) void pairsKernel(const uint32_t *mapped, const uint32_t *id, const uint32_t *numSurvivors, uint32_t b,
                                                   uint64_t *keys)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *numSurvivors)
        return;
    const uint64_t t = id[i];
    keys[i] = (uint64_t) mapped[3 * t] << b | mapped[3 * t + 1];
}

/* the survivors in (first, second, third) order: one of a run of equal triples is kept */
struct UniqueIn
{
    const uint64_t *keys;
    const uint32_t *id, *mapped;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        if (i == 0)
            return 1u;
        const uint64_t key = keys[i], keyBefore = keys[i - 1];
        const uint64_t t = id[i], tBefore = id[i - 1];
        return key != keyBefore || mapped[3 * t + 2] != mapped[3 * tBefore + 2] ? 1u : 0u;
    }
};
struct UniqueOut
{
    const uint64_t *keys;
    const uint32_t *id, *mapped;
    uint32_t b;
    uint32_t *outTriangles, *used;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t before, uint32_t kept) const
    {
        if (!kept)
            return;
        const uint64_t key = keys[i];
        const uint32_t first = (uint32_t) (key >> b), second = (uint32_t) (key & ((uint64_t(1) << b) - 1));
        const uint32_t third = mapped[3 * (uint64_t) id[i] + 2];
        outTriangles[3 * (uint64_t) before] = first;
        outTriangles[3 * (uint64_t) before + 1] = second;
        outTriangles[3 * (uint64_t) before + 2] = third;
        used[first] = 1u;       /* plain stores that race only with stores of the same value */
        used[second] = 1u;
        used[third] = 1u;
    }
};

/* steps 3 (second half) and 5: the used clusters in key order are the output vertices */
struct UsedIn
{
    const uint32_t *used;
    __device__ __forceinline__ uint32_t operator()(uint64_t c) const { return used[c]; }
};
struct VertexOut
{
    const float *vertices;
    const uint64_t *sortedKeys;
    const uint32_t *sortedVertex, *start;
    const Counter *sums;
    Frame F;
    KeyBits bits;
    uint32_t *newIndex;         /* the array UsedIn reads: an element is read by the thread that writes it, before */
    float *outVertices;
    __device__ __forceinline__ void operator()(uint64_t cluster, uint32_t before, uint32_t isUsed) const
    {
        newIndex[cluster] = before;
        if (!isUsed)
            return;
        const uint32_t first = start[cluster], members = start[cluster + 1] - first;
        float out[3];
        if (members == 1)
        {
            const uint64_t v = sortedVertex[first];
#pragma unroll
            for (int k = 0; k < 3; k++)
                out[k] = vertices[3 * v + k];
        }
        else
        {
            uint32_t c[3];
            bits.unpack(sortedKeys[first], c);
#pragma unroll
            for (int k = 0; k < 3; k++)
            {
                const long long S = (long long) sums[3 * cluster + k];
                const double mean = ((double) S / (double) members) * (1.0 / FIXED_ONE);
                out[k] = (float) ((double) F.origin[k] + ((double) c[k] + mean) * (double) F.cellSize);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; k++)
            outVertices[3 * (uint64_t) before + k] = out[k];
    }
};

/* ---- quadric placement ---- */

/* steps 3b and 3c of the quadric contract for triangle t, whose indices are in range: g per corner, n = (g1 - g0) x (g2 - g0)
 * in normals.hip's operation order */
struct CellFace
{
    uint32_t index[3];
    double g[3][3], n[3];
};
__device__ __forceinline__ CellFace cellFaceOf(const float *vertices, const uint32_t index[3], const Frame &F)
{
    CellFace f;
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        f.index[k] = index[k];
#pragma unroll
        for (int axis = 0; axis < 3; axis++)
            f.g[k][axis] = ((double) vertices[3 * (uint64_t) index[k] + axis] - (double) F.origin[axis]) / (double) F.cellSize;
    }
    double a[3], b[3];
#pragma unroll
    for (int axis = 0; axis < 3; axis++)
    {
        a[axis] = f.g[1][axis] - f.g[0][axis];
        b[axis] = f.g[2][axis] - f.g[0][axis];
    }
    f.n[0] = a[1] * b[2] - a[2] * b[1];
    f.n[1] = a[2] * b[0] - a[0] * b[2];
    f.n[2] = a[0] * b[1] - a[1] * b[0];
    return f;
}

/* Runs before the read-back that validates the mesh: an index >= V is skipped here (and refuses the call there), and what a
 * vertex that is not valid leaves in the maximum is never used.  Every lane of every wave stays to the end: waveMax64 needs
 * the full wave. */
__global__ __launch_bounds__(256) void extentKernel(const float *vertices, uint64_t numVertices, const uint32_t *triangles,
                                                    uint64_t numTriangles, Frame F, Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t bits = 0;
    if (t < numTriangles)
    {
        const uint32_t index[3] = {triangles[3 * t], triangles[3 * t + 1], triangles[3 * t + 2]};
        if (index[0] < numVertices && index[1] < numVertices && index[2] < numVertices)
        {
            const CellFace f = cellFaceOf(vertices, index, F);
            bits = (uint64_t) __double_as_longlong(fmax(fmax(fabs(f.n[0]), fabs(f.n[1])), fabs(f.n[2])));
        }
    }
    /* the word is read first, as meshpost.hpp's foldMax does: the first few waves reach the maximum, and the 60 000 waves of a
     * 4 M-triangle chunk would otherwise queue at one address (0.68 ms against 0.07 ms, profiles/NOTES_simplify_quadric.md) */
    const uint64_t most = waveMax64(bits);
    if (laneId() == 0 && (Counter) most > __hip_atomic_load(&counters[C_MAX_BITS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(&counters[C_MAX_BITS], (Counter) most);
}

/* q of step 3e: ldexp is exact wherever the result is normal, and a result that is not is far below 1/2; rint rounds ties to
 * even; |x| < 2^(E + 2), so |q| <= 2^(s + 2) <= 2^61 */
__device__ __forceinline__ long long quantiseProduct(double x, int shift)
{
    return (long long) rint(ldexp(x, shift));
}

/* One corner slot of the wave: the lanes whose `cluster` is not NO_CLUSTER add their nine q (zero in the other lanes) to that
 * cluster's sums.  WAVE_COMBINED: a wave whose adding lanes all name one cluster (the inside of a large cluster) adds up by
 * butterflies and sends once; otherwise runs of equal clusters among neighbouring lanes (marching emits triangles in spatial
 * order) add up by shuffles and the run's first lane sends; a wave without two equal neighbours sends lane by lane, as every
 * wave does without WAVE_COMBINED.  A sum of zero is not sent.  The sums are integers: every route gives the same bits.
 * The full wave calls this. */
template<bool WAVE_COMBINED>
__device__ __forceinline__ void addToClusters(uint32_t cluster, const long long (&q)[QUADRIC_SUMS], Counter *sums)
{
    const bool adds = cluster != NO_CLUSTER;
    if (WAVE_COMBINED)
    {
        const uint64_t adders = __ballot(adds);
        if (adders == 0)
            return;             /* (wave-uniform) */
        const uint32_t lane = laneId();
        const uint32_t firstCluster = readLane(cluster, (int) __builtin_ctzll(adders));
        if (__ballot(adds && cluster != firstCluster) == 0)
        {
#pragma unroll
            for (int k = 0; k < QUADRIC_SUMS; k++)
            {
                const long long s = waveSum64(q[k]);
                if (lane == 0 && s != 0)
                    atomicAdd(&sums[QUADRIC_SUMS * (uint64_t) firstCluster + k], (Counter) s);
            }
            return;
        }
        const uint32_t before = waveShiftUp1(cluster);
        const bool head = lane == 0 || before != cluster || !adds;
        if (__ballot(!head) != 0)
        {
            const uint32_t run = waveInclusiveScan(head ? 1u : 0u);
            long long s[QUADRIC_SUMS];
#pragma unroll
            for (int k = 0; k < QUADRIC_SUMS; k++)
                s[k] = q[k];
#pragma unroll
            for (int step = 1; step < WAVE; step <<= 1)
            {
                const bool same = __shfl_down(run, step, WAVE) == run && lane + step < WAVE;
#pragma unroll
                for (int k = 0; k < QUADRIC_SUMS; k++)
                {
                    const long long other = __shfl_down(s[k], step, WAVE);
                    s[k] += same ? other : 0;
                }
            }
            if (head && adds)
#pragma unroll
                for (int k = 0; k < QUADRIC_SUMS; k++)
                    if (s[k] != 0)
                        atomicAdd(&sums[QUADRIC_SUMS * (uint64_t) cluster + k], (Counter) s[k]);
            return;
        }
    }
    if (adds)
#pragma unroll
        for (int k = 0; k < QUADRIC_SUMS; k++)
            if (q[k] != 0)
                atomicAdd(&sums[QUADRIC_SUMS * (uint64_t) cluster + k], (Counter) q[k]);
}

/* Step 3e.  Every vertex and every index is valid: the read-back said so.  No lane leaves before the shuffles. */
template<bool WAVE_COMBINED>
__global__ __launch_bounds__(256) void quadricsKernel(const float *vertices, const uint32_t *triangles, uint64_t numTriangles,
                                                      const uint32_t *clusterOfVertex, Frame F, int shift, Counter *sums)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = t < numTriangles;
    uint32_t cluster[3] = {NO_CLUSTER, NO_CLUSTER, NO_CLUSTER};
    double n[3] = {0.0, 0.0, 0.0}, w[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if (live)
    {
        const uint32_t index[3] = {triangles[3 * t], triangles[3 * t + 1], triangles[3 * t + 2]};
        const CellFace f = cellFaceOf(vertices, index, F);
#pragma unroll
        for (int k = 0; k < 3; k++)
        {
            const float p[3] = {vertices[3 * (uint64_t) index[k]], vertices[3 * (uint64_t) index[k] + 1],
                                vertices[3 * (uint64_t) index[k] + 2]};
            uint32_t c[3];
            cellOf(p, F, c);
#pragma unroll
            for (int axis = 0; axis < 3; axis++)
                w[k][axis] = (f.g[k][axis] - (double) c[axis]) - 0.5;
            cluster[k] = clusterOfVertex[index[k]];
        }
#pragma unroll
        for (int axis = 0; axis < 3; axis++)
            n[axis] = f.n[axis];
        /* once per distinct cluster: corner k adds iff its cluster differs from those of the corners before it */
        if (cluster[2] == cluster[0] || cluster[2] == cluster[1])
            cluster[2] = NO_CLUSTER;
        if (cluster[1] == cluster[0])
            cluster[1] = NO_CLUSTER;
    }
    long long q[QUADRIC_SUMS];
    q[0] = quantiseProduct(n[0] * n[0], shift);
    q[1] = quantiseProduct(n[0] * n[1], shift);
    q[2] = quantiseProduct(n[0] * n[2], shift);
    q[3] = quantiseProduct(n[1] * n[1], shift);
    q[4] = quantiseProduct(n[1] * n[2], shift);
    q[5] = quantiseProduct(n[2] * n[2], shift);
#pragma unroll
    for (int k = 0; k < 3; k++)
    {
        const double d = -((n[0] * w[k][0] + n[1] * w[k][1]) + n[2] * w[k][2]);
        long long mine[QUADRIC_SUMS];
#pragma unroll
        for (int j = 0; j < 6; j++)
            mine[j] = cluster[k] != NO_CLUSTER ? q[j] : 0;
#pragma unroll
        for (int axis = 0; axis < 3; axis++)
            mine[6 + axis] = cluster[k] != NO_CLUSTER ? quantiseProduct(d * n[axis], shift) : 0;
        addToClusters<WAVE_COMBINED>(cluster[k], mine, sums);
    }
}

/* Steps 3f to 3h in VertexOut's place: a used cluster of several members is solved; where that falls back, and for every
 * other cluster, VertexOut does what it does for the mean variant, so that those bits are its bits. */
struct QuadricOut
{
    VertexOut mean;
    const Counter *quadrics;    /* [clusters][QUADRIC_SUMS] */
    Counter *counters;
    __device__ __forceinline__ void operator()(uint64_t cluster, uint32_t before, uint32_t isUsed) const
    {
        bool solved = false, flat = false, escaped = false;
        double x[3] = {0.0, 0.0, 0.0};
        uint32_t first = 0;
        if (isUsed)
        {
            first = mean.start[cluster];
            const uint32_t members = mean.start[cluster + 1] - first;
            if (members > 1)
            {
                double a[6], b[3], m[3];
#pragma unroll
                for (int k = 0; k < 6; k++)
                    a[k] = (double) (long long) quadrics[QUADRIC_SUMS * cluster + k];
#pragma unroll
                for (int k = 0; k < 3; k++)
                {
                    b[k] = (double) (long long) quadrics[QUADRIC_SUMS * cluster + 6 + k];
                    const long long S = (long long) mean.sums[3 * cluster + k];
                    m[k] = ((double) S / (double) members) * (1.0 / FIXED_ONE) - 0.5;
                }
                const double tr = (a[0] + a[3]) + a[5];
                flat = tr == 0.0;
                if (!flat)
                {
                    const double mu = tr * (1.0 / 1024.0);
                    const double r0 = mu * m[0] - b[0], r1 = mu * m[1] - b[1], r2 = mu * m[2] - b[2];
                    const double d0 = a[0] + mu, l10 = a[1] / d0, l20 = a[2] / d0;
                    const double d1 = (a[3] + mu) - l10 * a[1], t = a[4] - l20 * a[1], l21 = t / d1;
                    const double d2 = ((a[5] + mu) - l20 * a[2]) - l21 * t;
                    const double y0 = r0, y1 = r1 - l10 * y0, y2 = (r2 - l20 * y0) - l21 * y1;
                    const double z0 = y0 / d0, z1 = y1 / d1, z2 = y2 / d2;
                    x[2] = z2;
                    x[1] = z1 - l21 * x[2];
                    x[0] = (z0 - l10 * x[1]) - l20 * x[2];
                    solved = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && fabs(x[0]) <= 0.5 && fabs(x[1]) <= 0.5
                             && fabs(x[2]) <= 0.5;
                    escaped = !solved;
                }
            }
        }
        tally(solved, &counters[C_SOLVED]);
        tally(flat, &counters[C_FLAT]);
        tally(escaped, &counters[C_ESCAPED]);
        if (!solved)
        {
            mean(cluster, before, isUsed);
            return;
        }
        mean.newIndex[cluster] = before;
        uint32_t c[3];
        mean.bits.unpack(mean.sortedKeys[first], c);
#pragma unroll
        for (int k = 0; k < 3; k++)
            mean.outVertices[3 * (uint64_t) before + k] =
                (float) ((double) mean.F.origin[k] + (((double) c[k] + 0.5) + x[k]) * (double) mean.F.cellSize);
    }
};

/* MLSGPU_HIP_SIMPLIFY_ACCUMULATE=plain|wave picks the quadrics kernel (same bits either way) */
bool waveAccumulateWanted()
{
    const char *e = getenv("MLSGPU_HIP_SIMPLIFY_ACCUMULATE");
    return e == nullptr || std::strcmp(e, "plain") != 0;
}

__global__ __launch_bounds__(256) void reindexKernel(uint32_t *outTriangles, const uint32_t *numOutTriangles, const uint32_t *newIndex)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * (uint64_t) *numOutTriangles)
        return;
    outTriangles[i] = newIndex[outTriangles[i]];
}

/* Both entry points.  *stats takes the six shared statistics; `quadric` is null for PLACE_MEAN, whose launches, scratch and
 * read-backs are what they were before there was a second placement. */
int simplifyMesh(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles, uint64_t numTriangles,
                 const float origin[3], float cellSize, float *dOutVertices, uint32_t *dOutTriangles, Placement placement,
                 mlsgpu_simplify_stats *stats, mlsgpu_simplify_quadric_stats *quadric)
{
    REQUIRE(ctx != nullptr && stats != nullptr && origin != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(cellSize) && cellSize > 0.0f, MLSGPU_ERR_INVALID);
    REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), MLSGPU_ERR_INVALID);
    /* the sorts' values and tile counts are 32-bit, and so are the indices of a triangle */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || (dVertices != nullptr && dOutVertices != nullptr), MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || (dTriangles != nullptr && dOutTriangles != nullptr), MLSGPU_ERR_INVALID);
    if (quadric != nullptr)
        std::memset(quadric, 0, sizeof(*quadric));      /* (stats is its head) */
    std::memset(stats, 0, sizeof(*stats));
    stats->inVertices = numVertices;
    stats->inTriangles = numTriangles;
    if (numVertices == 0 && numTriangles == 0)
        return MLSGPU_OK;

    HIP_CHECK(hipSetDevice(ctx->device));
    const uint64_t nv = numVertices, nt = numTriangles, most = std::max(nv, nt);
    const Frame F = {{origin[0], origin[1], origin[2]}, cellSize};
    const dim3 B(256);
    const bool quadrics = placement == PLACE_QUADRIC;
    const uint64_t numCounters = quadrics ? C_QUADRIC_WORDS : C_WORDS;
    DeviceArray<Counter> counters;
    DeviceArray<uint32_t> words;
    PROPAGATE(counters.alloc(numCounters));
    PROPAGATE(words.alloc(W_WORDS));
    HIP_CHECK(hipMemsetAsync(counters.get(), 0, numCounters * sizeof(Counter), ctx->stream));
    HIP_CHECK(hipMemsetAsync(words.get(), 0, W_WORDS * sizeof(uint32_t), ctx->stream));
    if (nv > 0)
        LAUNCH(ctx, "kernel.simplify.bounds", boundsKernel, dim3(divUp(nv, 256)), B, dVertices, nv, F, counters.get(), words.get());
    if (nt > 0)
        LAUNCH(ctx, "kernel.simplify.indices", indicesKernel, dim3(divUp(3 * nt, 256)), B, dTriangles, 3 * nt, nv, counters.get());
    /* the scale of the quadrics is read back with the errors, so that the quadric placement adds no synchronisation */
    if (quadrics && nt > 0 && nv > 0)
        LAUNCH(ctx, "kernel.simplify.extent", extentKernel, dim3(divUp(nt, 256)), B, dVertices, nv, dTriangles, nt, F, counters.get());
    Counter hCounters[C_QUADRIC_WORDS] = {};
    uint32_t hWords[W_WORDS];
    HIP_CHECK(hipMemcpyAsync(hCounters, counters.get(), numCounters * sizeof(Counter), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(hWords, words.get(), sizeof(hWords), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (hCounters[C_BAD_VERTICES] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh simplify: %llu vertices are not finite or lie outside the 2^21 cells per axis",
                        hCounters[C_BAD_VERTICES]);
    if (hCounters[C_BAD_INDICES] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh simplify: %llu triangle indices are out of range", hCounters[C_BAD_INDICES]);
    if (nv == 0 || nt == 0)
        return MLSGPU_OK;       /* an empty mesh */

    const KeyBits bits = {bitLength(hWords[W_MAX_CELL]), bitLength(hWords[W_MAX_CELL + 1]), bitLength(hWords[W_MAX_CELL + 2])};
    const uint32_t b = bitLength(nv);           /* a cluster is < V */
    DeviceArray<uint64_t> vKeysA, vKeysB, tKeysA, tKeysB;
    DeviceArray<uint32_t> vValsA, vValsB, hist, tileSums, clusterOfVertex, start, used, mapped, thirdA, thirdB, tValsA, tValsB;
    DeviceArray<Counter> sums;
    const uint64_t histElems = sortHistElems(most), tileElems = (uint64_t) scanTiles(most) + 1;
    PROPAGATE(vKeysA.alloc(nv));
    PROPAGATE(vKeysB.alloc(nv));
    PROPAGATE(vValsA.alloc(nv));
    PROPAGATE(vValsB.alloc(nv));
    PROPAGATE(clusterOfVertex.alloc(nv));
    PROPAGATE(start.alloc(nv + 1));
    const uint64_t sumWords = (quadrics ? 3 + QUADRIC_SUMS : 3) * nv;         /* the mean's three per cluster, then the quadrics' nine */
    PROPAGATE(sums.alloc(sumWords));
    PROPAGATE(used.alloc(nv));
    PROPAGATE(mapped.alloc(3 * nt));
    PROPAGATE(thirdA.alloc(nt));
    PROPAGATE(thirdB.alloc(nt));
    PROPAGATE(tValsA.alloc(nt));
    PROPAGATE(tValsB.alloc(nt));
    PROPAGATE(tKeysA.alloc(nt));
    PROPAGATE(tKeysB.alloc(nt));
    PROPAGATE(hist.alloc(histElems));
    PROPAGATE(tileSums.alloc(tileElems));
    if (ctx->timing)
        ctx->addValue("simplify.scratch.bytes",
                      (double) (2 * vKeysA.bytes(nv) + 4 * vValsA.bytes(nv) + start.bytes(nv + 1) + sums.bytes(sumWords)
                                + mapped.bytes(3 * nt) + 4 * thirdA.bytes(nt) + 2 * tKeysA.bytes(nt) + hist.bytes(histElems)
                                + tileSums.bytes(tileElems) + counters.bytes(numCounters) + words.bytes(W_WORDS)));
    uint32_t *const dWords = words.get();

    /* clusters */
    LAUNCH(ctx, "kernel.simplify.keys", keysKernel, dim3(divUp(nv, 256)), B, dVertices, nv, F, bits, vKeysA.get());
    SortResult<uint64_t> sv = {nullptr, nullptr};
    PROPAGATE(radixSort<uint64_t>(ctx, "kernel.simplify.sortVertices", vKeysA, vValsA, vKeysB, vValsB, nv, bits.x + bits.y + bits.z,
                                  true, hist, nullptr, &sv));
    /* the side of the sort that does not hold the result is free again: the cluster of every sorted position */
    uint32_t *const clusterOfPosition = sv.vals == vValsA.get() ? vValsB.get() : vValsA.get();
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.clusters", HeadIn{sv.keys},
                                       ClusterOut{sv.vals, clusterOfVertex, clusterOfPosition, start, nv}, nv, 0u, tileSums.get(),
                                       dWords + W_CLUSTERS)));
    HIP_CHECK(hipMemsetAsync(sums.get(), 0, sumWords * sizeof(Counter), ctx->stream));
    HIP_CHECK(hipMemsetAsync(used.get(), 0, nv * sizeof(uint32_t), ctx->stream));
    LAUNCH(ctx, "kernel.simplify.sums", sumsKernel, dim3(divUp(nv, 256)), B, dVertices, (const uint64_t *) sv.keys,
           (const uint32_t *) sv.vals, (const uint32_t *) clusterOfPosition, nv, F, bits, sums.get());
    Counter *const quadricSums = sums.get() + 3 * nv;
    const uint64_t maxBits = hCounters[C_MAX_BITS];     /* zero for the mean */
    if (maxBits != 0)
    {
        /* step 3d: products below 2^(E + 1), s = 60 - bitLength(T) bits of them kept */
        const int E = 2 * exponentOfDoubleBits(maxBits) + 1, shift = 60 - (int) bitLength(nt) - E;
        quadric->scaleExponent = E;
        if (waveAccumulateWanted())
            LAUNCH(ctx, "kernel.simplify.quadrics", quadricsKernel<true>, dim3(divUp(nt, 256)), B, dVertices, dTriangles, nt,
                   (const uint32_t *) clusterOfVertex.get(), F, shift, quadricSums);
        else
            LAUNCH(ctx, "kernel.simplify.quadrics", quadricsKernel<false>, dim3(divUp(nt, 256)), B, dVertices, dTriangles, nt,
                   (const uint32_t *) clusterOfVertex.get(), F, shift, quadricSums);
    }

    /* triangles */
    LAUNCH(ctx, "kernel.simplify.map", mapKernel, dim3(divUp(nt, 256)), B, dTriangles, nt, nv, (const uint32_t *) clusterOfVertex.get(),
           mapped.get(), counters.get());
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.survivors", SurvivorIn{mapped}, SurvivorOut{mapped, thirdA, tValsA}, nt, 0u,
                                       tileSums.get(), dWords + W_SURVIVORS)));
    const uint32_t *const dSurvivors = dWords + W_SURVIVORS;
    SortResult<uint32_t> byThird = {nullptr, nullptr};
    PROPAGATE(radixSort<uint32_t>(ctx, "kernel.simplify.sortTriangles", thirdA, tValsA, thirdB, tValsB, nt, b, false, hist, nullptr,
                                  &byThird, dSurvivors));
    uint32_t *const idsOther = byThird.vals == tValsA.get() ? tValsB.get() : tValsA.get();
    LAUNCH(ctx, "kernel.simplify.pairs", pairsKernel, dim3(divUp(nt, 256)), B, (const uint32_t *) mapped.get(),
           (const uint32_t *) byThird.vals, dSurvivors, b, tKeysA.get());
    SortResult<uint64_t> ordered = {nullptr, nullptr};
    PROPAGATE(radixSort<uint64_t>(ctx, "kernel.simplify.sortTriangles", tKeysA.get(), byThird.vals, tKeysB.get(), idsOther, nt, 2 * b,
                                  false, hist, nullptr, &ordered, dSurvivors));
    PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.unique", UniqueIn{ordered.keys, ordered.vals, mapped},
                                       UniqueOut{ordered.keys, ordered.vals, mapped, b, dOutTriangles, used}, nt, 0u, tileSums.get(),
                                       dWords + W_OUT_TRIANGLES, dSurvivors)));

    /* output */
    const VertexOut atMean = {dVertices, sv.keys, sv.vals, start, sums, F, bits, used, dOutVertices};
    if (quadrics)
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.vertices", UsedIn{used},
                                           QuadricOut{atMean, quadricSums, counters.get()}, nv, 0u, tileSums.get(),
                                           dWords + W_OUT_VERTICES, (const uint32_t *) (dWords + W_CLUSTERS))));
    else
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.simplify.vertices", UsedIn{used}, atMean, nv, 0u, tileSums.get(),
                                           dWords + W_OUT_VERTICES, (const uint32_t *) (dWords + W_CLUSTERS))));
    LAUNCH(ctx, "kernel.simplify.reindex", reindexKernel, dim3(divUp(3 * nt, 256)), B, dOutTriangles,
           (const uint32_t *) (dWords + W_OUT_TRIANGLES), (const uint32_t *) used.get());

    HIP_CHECK(hipMemcpyAsync(hCounters, counters.get(), numCounters * sizeof(Counter), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(hWords, words.get(), sizeof(hWords), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    stats->outVertices = hWords[W_OUT_VERTICES];
    stats->outTriangles = hWords[W_OUT_TRIANGLES];
    stats->collapsedTriangles = hCounters[C_COLLAPSED];
    stats->duplicateTriangles = (uint64_t) hWords[W_SURVIVORS] - hWords[W_OUT_TRIANGLES];
    if (quadrics)
    {
        quadric->solvedVertices = hCounters[C_SOLVED];
        quadric->flatVertices = hCounters[C_FLAT];
        quadric->escapedVertices = hCounters[C_ESCAPED];
    }
    return MLSGPU_OK;
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_simplify(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                        uint64_t numTriangles, const float origin[3], float cellSize, float *dOutVertices,
                                        uint32_t *dOutTriangles, mlsgpu_simplify_stats *stats)
{
    return simplifyMesh(ctx, dVertices, numVertices, dTriangles, numTriangles, origin, cellSize, dOutVertices, dOutTriangles,
                        PLACE_MEAN, stats, nullptr);
}

/* the six shared statistics are the head of mlsgpu_simplify_quadric_stats, field for field */
static_assert(offsetof(mlsgpu_simplify_quadric_stats, solvedVertices) == sizeof(mlsgpu_simplify_stats),
              "mlsgpu_simplify_quadric_stats begins with mlsgpu_simplify_stats");

MLSGPU_API int mlsgpu_hip_mesh_simplify_quadric(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices,
                                                const uint32_t *dTriangles, uint64_t numTriangles, const float origin[3],
                                                float cellSize, float *dOutVertices, uint32_t *dOutTriangles,
                                                mlsgpu_simplify_quadric_stats *stats)
{
    return simplifyMesh(ctx, dVertices, numVertices, dTriangles, numTriangles, origin, cellSize, dOutVertices, dOutTriangles,
                        PLACE_QUADRIC, reinterpret_cast<mlsgpu_simplify_stats *>(stats), stats);
}
