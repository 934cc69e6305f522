/*
 * The self-intersection report of an indexed triangle mesh resident in HBM: which pairs of triangles certainly pass through
 * each other.  The reference has no counterpart.  The contract (include/mlsgpu_hip.h, DESIGN.md "Mesh self-intersections")
 * fixes every floating-point operation and makes every field of the report a count, a minimum or a maximum: the result depends
 * neither on the schedule nor on anything below that the contract does not name -- the grid's cell size least of all.
 *
 *   grid       the triangles that take part (step 1), each in the cells its box touches, as (cell key, triangle) records
 *              sorted by cell key: meshgrid.hpp, with reach = 0 and the cell of every triangle's lower corner kept
 *   pairs      over the sorted records: a lane owns record i and meets the later records of the same cell; steps 2 to 5 for
 *              each pair that this cell owns                                                       -- one read-back --
 *   list       (where the caller takes the pairs and they fit) the same walk once more, over the triangles that have a
 *              partner only, appending the crossing pairs packed A << 32 | B; one sort; one kernel that unpacks them
 *   report     over the partner counts: the triangles that have one, the maximum; then the lowest triangle that attains it
 *                                                                                                   -- one read-back --
 *
 * Why a pair is met exactly once.  cell() is monotone (meshgrid.hpp), and a triangle goes into every cell from cell(lo) to
 * cell(hi) per axis.  For a candidate pair loA <= hiB and loB <= hiA, so m = max(cell(loA), cell(loB)) lies within cell(lo) ..
 * cell(hi) of both on every axis: both have a record in cell m, and the pair is looked at there and nowhere else -- no atomics
 * to deduplicate, no second sort.  A pair that is no candidate may meet in m or not at all; step 2 drops it.
 *
 * A record's triangle is classified again before its corners are read: an index >= V is never an address here either.
 *
 * Scratch belongs to the call: 16 bytes per triangle (its cell count, where its records begin, the packed cell of its lower
 * corner) and 4 more where the caller does not take the partner counts, 24 bytes per grid record (the two sides of the sort's
 * 64-bit keys and 32-bit values), 24 bytes per crossing pair where the list is written, the sorts' histograms (4 KB per 4096
 * records) and the scan's tile sums.  The records are at most max(2^20, 8 T).
 */
#include "meshgrid.hpp"

#include <cmath>
#include <cstdlib>

using namespace mlsgpu;

namespace
{

enum
{
    C_CANDIDATES = G_WORDS,
    C_CROSSINGS,
    C_LOWEST,                   /* a minimum: the lowest crossing pair, packed */
    C_CURSOR,                   /* the list pass: pairs appended */
    C_CROSSING_TRIANGLES,
    C_MAX_PARTNERS,
    C_MAX_TRIANGLE,             /* a minimum: the lowest triangle with C_MAX_PARTNERS partners */
    C_MAX_TIES,                 /* the triangles that attain the maximum (tally() counts what it finds the first of) */
    C_TESTED,                   /* a timed call: the record pairs the pairs kernel looked at */
    C_WORDS
};

const GridNames NAMES = {"mesh self-intersections", "records", "kernel.intersect.extent", "kernel.intersect.classify",
                         "kernel.intersect.count", "kernel.intersect.scan", "kernel.intersect.emit", "kernel.intersect.sort",
                         "intersect.records", "intersect.cellsize"};

const uint32_t OWN_STEPS = 32;                  /* the later records a lane meets alone, before the wave shares the rest */
const double FILTER = 3.552713678800501e-15;    /* 2^-48 (step 3) */

/* per axis the larger of two packed cells (packCell(): z << 42 | y << 21 | x) */
__device__ __forceinline__ uint64_t largerCell(uint64_t p, uint64_t q)
{
    const uint64_t M = (uint64_t(1) << 21) - 1;
    return max(p >> 42, q >> 42) << 42 | max((p >> 21) & M, (q >> 21) & M) << 21 | max(p & M, q & M);
}

struct F3
{
    float x, y, z;
};
struct Corners
{
    F3 a, b, c;
};

/* the corners of a triangle whose indices i, j, k are known to be in range */
__device__ __forceinline__ Corners cornersOf(const float *vertices, uint64_t i, uint64_t j, uint64_t k)
{
    Corners T;
    T.a = F3{vertices[3 * i], vertices[3 * i + 1], vertices[3 * i + 2]};
    T.b = F3{vertices[3 * j], vertices[3 * j + 1], vertices[3 * j + 2]};
    T.c = F3{vertices[3 * k], vertices[3 * k + 1], vertices[3 * k + 2]};
    return T;
}

struct Box
{
    float lo[3], hi[3];
};
__device__ __forceinline__ Box boxOf(const Corners &T)
{
    Box B;
    B.lo[0] = fminf(fminf(T.a.x, T.b.x), T.c.x);
    B.hi[0] = fmaxf(fmaxf(T.a.x, T.b.x), T.c.x);
    B.lo[1] = fminf(fminf(T.a.y, T.b.y), T.c.y);
    B.hi[1] = fmaxf(fmaxf(T.a.y, T.b.y), T.c.y);
    B.lo[2] = fminf(fminf(T.a.z, T.b.z), T.c.z);
    B.hi[2] = fmaxf(fmaxf(T.a.z, T.b.z), T.c.z);
    return B;
}

/* ---------------------------------------------------------------- steps 3 to 5 */

struct D3
{
    double x, y, z;
};
__device__ __forceinline__ D3 sub(const D3 &u, const D3 &v) { return D3{u.x - v.x, u.y - v.y, u.z - v.z}; }
__device__ __forceinline__ D3 widen(const F3 &f) { return D3{(double) f.x, (double) f.y, (double) f.z}; }
__device__ __forceinline__ F3 pick(int k, const F3 &a, const F3 &b, const F3 &c)
{
    return F3{k == 0 ? a.x : k == 1 ? b.x : c.x, k == 0 ? a.y : k == 1 ? b.y : c.y, k == 0 ? a.z : k == 1 ? b.z : c.z};
}

/* Step 3: det = dot(a - x, cross(b - x, c - x)) and the same sum over absolute values; the products of the cross are shared.
 * The corners come as floats and are widened here (exactly), where they are used: eighteen doubles that stay in registers
 * across the whole predicate cost the kernel its occupancy (profiles/NOTES_intersect.md). */
__device__ __forceinline__ int orient(const F3 &a, const F3 &b, const F3 &c, const F3 &x)
{
    const D3 X = widen(x);
    const D3 r0 = sub(widen(a), X), r1 = sub(widen(b), X), r2 = sub(widen(c), X);
    const double yz = r1.y * r2.z, zy = r1.z * r2.y;
    const double zx = r1.z * r2.x, xz = r1.x * r2.z;
    const double xy = r1.x * r2.y, yx = r1.y * r2.x;
    const double det = (r0.x * (yz - zy) + r0.y * (zx - xz)) + r0.z * (xy - yx);
    const double perm = (fabs(r0.x) * (fabs(yz) + fabs(zy)) + fabs(r0.y) * (fabs(zx) + fabs(xz))) + fabs(r0.z) * (fabs(xy) + fabs(yx));
    return fabs(det) <= perm * FILTER ? 0 : (det > 0.0 ? 1 : -1);
}

/* Steps 4 and 5: does a side of S pierce T or a side of T pierce S.  Every orient() is a function of its arguments alone, so
 * the three side signs are worked out only where the plane signs differ: what is left out cannot change the answer.  The two
 * directions and the three sides are loops that are NOT unrolled, so that the kernel holds six orient() and not twenty-four
 * whose common differences the compiler would keep in registers all along.  S and T change places behind each direction:
 * behind the second they are back where they were. */
__device__ __forceinline__ bool crosses(Corners &S, Corners &T)
{
    bool hit = false;
#pragma unroll 1
    for (int direction = 0; direction < 2; direction++)
    {
        const int above0 = orient(T.a, T.b, T.c, S.a), above1 = orient(T.a, T.b, T.c, S.b), above2 = orient(T.a, T.b, T.c, S.c);
#pragma unroll 1
        for (int k = 0; k < 3; k++)
        {
            const int from = k == 0 ? above0 : k == 1 ? above1 : above2, to = k == 0 ? above1 : k == 1 ? above2 : above0;
            if (from * to < 0)
            {
                const F3 p = pick(k, S.a, S.b, S.c), q = pick(k, S.b, S.c, S.a);
                const int s0 = orient(p, q, T.a, T.b);
                const int s1 = orient(p, q, T.b, T.c);
                const int s2 = orient(p, q, T.c, T.a);
                hit = hit || (s0 != 0 && s0 == s1 && s1 == s2);
            }
        }
        const Corners C = S;
        S = T;
        T = C;
    }
    return hit;
}

/* ---------------------------------------------------------------- kernels */

/* what the pairs kernel reads and writes */
struct PairsArgs
{
    Grid G;
    const float *vertices;
    uint64_t numVertices;
    const uint32_t *tri;
    uint64_t numTriangles;
    const uint64_t *lowerCell;
    const uint64_t *keys;       /* the sorted records */
    const uint32_t *vals;
    uint32_t numRecords;
    uint32_t *partners;         /* per triangle */
    uint64_t *list;             /* LIST: room for listCapacity packed pairs */
    uint64_t listCapacity;
    Counter *counters;
    bool tally;                 /* a timed call: count the record pairs looked at */
};

/* one end of a pair: the triangle of a record, classified again before its corners are read */
struct End
{
    uint32_t t;
    bool live;
    uint64_t lower;             /* the packed cell of its box's lower corner */
    Corners T;
    Box B;
};
/* `with`: the other end (its lower corner's cell) and the cell they meet in -- an end that the owning-cell rule keeps out of
 * this cell is done with after one 8-byte read, which is most of them */
template<bool LIST>
__device__ __forceinline__ End endOf(const PairsArgs &a, uint32_t record, const uint64_t *with = nullptr, uint64_t here = 0)
{
    End e;
    e.t = a.vals[record];
    e.live = false;
    e.lower = 0;
    if (e.t < a.numTriangles && !(LIST && a.partners[e.t] == 0)
        && (with == nullptr || largerCell(*with, a.lowerCell[e.t]) == here))
    {
        const uint64_t i[3] = {a.tri[3 * (uint64_t) e.t], a.tri[3 * (uint64_t) e.t + 1], a.tri[3 * (uint64_t) e.t + 2]};
        if (defectOf(i, a.numVertices).none())
        {
            e.live = true;
            e.lower = a.lowerCell[e.t];
            e.T = cornersOf(a.vertices, i[0], i[1], i[2]);
            e.B = boxOf(e.T);
        }
    }
    return e;
}

/* The pair of the records' triangles, met in the cell `here` (packed): the owning-cell rule, step 2, steps 3 to 5.  Without
 * LIST a crossing counts for both triangles and lowers the lowest pair; with LIST it is appended. */
template<bool LIST>
__device__ __forceinline__ void meet(const PairsArgs &a, End &A, uint64_t here, uint32_t record, long long *candidates,
                                     long long *crossings)
{
    End B = endOf<LIST>(a, record, &A.lower, here);
    if (!B.live)
        return;
    bool candidate = true;
#pragma unroll
    for (int x = 0; x < 3; x++)
        candidate = candidate && A.B.lo[x] <= B.B.hi[x] && B.B.lo[x] <= A.B.hi[x];
    if (!candidate)
        return;
    ++*candidates;
    if (!crosses(A.T, B.T))
        return;
    ++*crossings;
    const uint32_t low = min(A.t, B.t), high = max(A.t, B.t);
    const uint64_t packed = (uint64_t) low << 32 | high;
    if (LIST)
    {
        const uint64_t at = atomicAdd(&a.counters[C_CURSOR], (Counter) 1);
        if (at < a.listCapacity)
            a.list[at] = packed;
    }
    else
    {
        atomicAdd(&a.partners[low], 1u);
        atomicAdd(&a.partners[high], 1u);
        atomicMin(&a.counters[C_LOWEST], (Counter) packed);
    }
}

/* Steps 2 to 5 over the sorted records.  A lane owns record i and meets the later records of the same cell: the first
 * OWN_STEPS of them alone, which is all of them in an ordinary cell.  What is left of a long run (a fan's centre holds
 * thousands of triangles) the wave shares: owner after owner, its 64 lanes take every 64th of the remaining records, so that
 * no lane walks thousands of pairs while its neighbours idle.  A pair of records is a pair of triangles; the owning-cell
 * rule keeps all but one of the cells two triangles share from looking at it.  The two counts go through the workgroup:
 * a 64-bit sum per wave, added up in LDS, one atomic each.  Every lane stays to the end. */
template<bool LIST>
__global__ __launch_bounds__(256) void pairsKernel(PairsArgs a)
{
    __shared__ unsigned long long ofGroup[3];
    if (threadIdx.x < 3)
        ofGroup[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t thread = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool mine = thread < a.numRecords;
    const uint32_t i = mine ? (uint32_t) thread : 0u, lane = laneId();
    long long candidates = 0, crossings = 0, tested = 0;
    /* round 0: the lane's own record and the next OWN_STEPS; every later round: one owner's record in all lanes, and every
     * 64th of what that owner left.  One loop, so that the predicate is in the kernel once. */
    uint64_t key = mine ? a.keys[i] : 0;
    End A = endOf<LIST>(a, i);
    A.live = A.live && mine;
    uint64_t j = (uint64_t) i + 1, stride = 1;
    uint32_t steps = OWN_STEPS, next = 0;
    uint64_t pending = 0;
    for (bool own = true;; own = false)
    {
        const uint64_t here = a.G.packedOf(key);
        for (uint32_t step = 0; A.live && step < steps && j < a.numRecords && a.keys[j] == key; step++, j += stride)
        {
            tested++;
            meet<LIST>(a, A, here, (uint32_t) j, &candidates, &crossings);
        }
        if (own)
        {
            next = (uint32_t) j;        /* the first record this lane has not met; j <= numRecords < 2^32 */
            pending = __ballot(A.live && j < a.numRecords && a.keys[j] == key);
        }
        if (pending == 0)
            break;
        const int owner = __ffsll((unsigned long long) pending) - 1;
        pending &= pending - 1;
        const uint32_t record = (uint32_t) __shfl((int) i, owner, WAVE);
        key = a.keys[record];
        A = endOf<LIST>(a, record);                     /* one address for the wave */
        j = (uint64_t) (uint32_t) __shfl((int) next, owner, WAVE) + lane;
        stride = WAVE;
        steps = 0xFFFFFFFFu;
    }
    const long long candidatesOfWave = waveSum64(candidates), crossingsOfWave = waveSum64(crossings);
    const long long testedOfWave = a.tally ? waveSum64(tested) : 0;
    if (lane == 0)
    {
        if (candidatesOfWave != 0)
            atomicAdd(&ofGroup[0], (unsigned long long) candidatesOfWave);
        if (crossingsOfWave != 0)
            atomicAdd(&ofGroup[1], (unsigned long long) crossingsOfWave);
        if (testedOfWave != 0)
            atomicAdd(&ofGroup[2], (unsigned long long) testedOfWave);
    }
    __syncthreads();
    if (!LIST && threadIdx.x < 3 && ofGroup[threadIdx.x] != 0)
    {
        const int at[3] = {C_CANDIDATES, C_CROSSINGS, C_TESTED};
        atomicAdd(&a.counters[at[threadIdx.x]], (Counter) ofGroup[threadIdx.x]);
    }
}

/* the sorted packed pairs as rows (A, B) */
__global__ __launch_bounds__(256) void unpackKernel(const uint64_t *packed, uint64_t numPairs, uint32_t *rows)
{
    const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= numPairs)
        return;
    rows[2 * i] = (uint32_t) (packed[i] >> 32);
    rows[2 * i + 1] = (uint32_t) packed[i];
}

/* Step 6 but for the triangle that is named.  A workgroup loops over the partner counts and sends once; what one workgroup
 * counts fits 32 bits (T < 2^32). */
__global__ __launch_bounds__(256) void reportKernel(const uint32_t *partners, uint64_t numTriangles, Counter *counters)
{
    __shared__ GroupCounts<1, 1> totals;
    totals.clear();
    const int at[2] = {C_CROSSING_TRIANGLES, C_MAX_PARTNERS};
    uint32_t crossing = 0, most = 0;
    for (uint64_t base = (uint64_t) blockIdx.x * blockDim.x; base < numTriangles; base += (uint64_t) gridDim.x * blockDim.x)
    {
        const uint64_t t = base + threadIdx.x;
        const uint32_t n = t < numTriangles ? partners[t] : 0u;
        crossing += n != 0 ? 1u : 0u;
        most = max(most, n);
    }
    totals.add(0, crossing);
    totals.raise(0, most);
    totals.flush(counters, at);
}

/* the lowest triangle that attains the maximum: few do, so one atomic per wave that has one */
__global__ __launch_bounds__(256) void mostKernel(const uint32_t *partners, uint64_t numTriangles, Counter *counters)
{
    const uint64_t t = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool hit = t < numTriangles && counters[C_MAX_PARTNERS] != 0 && (Counter) partners[t] == counters[C_MAX_PARTNERS];
    tally(hit, &counters[C_MAX_TIES], t, &counters[C_MAX_TRIANGLE]);
}

} // namespace

MLSGPU_API int mlsgpu_hip_mesh_self_intersections(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices,
                                                  const uint32_t *dTriangles, uint64_t numTriangles, uint32_t *dPartners,
                                                  uint32_t *dPairs, uint64_t pairCapacity, mlsgpu_self_intersections *out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    /* the sort's values and the indices of a triangle are 32-bit */
    REQUIRE(numVertices < (uint64_t(1) << 32) && numTriangles < ((uint64_t(1) << 32) + 2) / 3, MLSGPU_ERR_LENGTH);
    REQUIRE(numVertices == 0 || dVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(numTriangles == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    const uint64_t nv = numVertices, nt = numTriangles;
    std::memset(out, 0, sizeof(*out));
    out->numVertices = nv;
    out->numTriangles = nt;
    out->lowestA = out->lowestB = out->maxPartnersTriangle = UINT64_MAX;

    HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 B(256);
    CounterBlock counters;
    PROPAGATE(counters.start(ctx, C_WORDS, {C_LOWEST, C_MAX_TRIANGLE}));
    const std::vector<Counter> &h = counters.h;
    TriangleGrid grid = {ctx, NAMES, counters, dVertices, nv, dTriangles, nt, 0.0};
    PROPAGATE(grid.measure(nullptr, 0, G_BAD_VERTICES));        /* no points: nothing is sent for them */
    if (grid.badVertices != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh self-intersections: %llu vertex coordinates are not finite",
                        (unsigned long long) grid.badVertices);
    out->outOfRangeTriangles = grid.outOfRange;
    out->degenerateTriangles = grid.degenerate;
    if (nt == 0)
        return MLSGPU_OK;

    DeviceArray<uint32_t> ownPartners;
    if (dPartners == nullptr)
    {
        PROPAGATE(ownPartners.alloc(nt));
        dPartners = ownPartners.get();
    }
    HIP_CHECK(hipMemsetAsync(dPartners, 0, nt * sizeof(uint32_t), ctx->stream));
    double scratch = (double) (counters.bytes() + (ownPartners.get() != nullptr ? ownPartners.bytes(nt) : 0));
    if (grid.live < 2)
    {
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (ctx->timing)
            ctx->addValue("intersect.scratch.bytes", scratch);
        return MLSGPU_OK;
    }

    SortScratch found;
    DeviceArray<uint64_t> lowerCell;
    PROPAGATE(lowerCell.alloc(nt));
    PROPAGATE(grid.build(grid.firstCell(), lowerCell.get()));
    scratch += (double) (grid.bytes() + lowerCell.bytes(nt));
    const uint64_t numRecords = grid.numRecords;
    PairsArgs args = {grid.G, dVertices, nv, dTriangles, nt, lowerCell.get(), grid.byCell.keys, grid.byCell.vals, (uint32_t) numRecords,
                      dPartners, nullptr, 0, counters.get(), ctx->timing != 0};
    LAUNCH(ctx, "kernel.intersect.pairs", (pairsKernel<false>), dim3(divUp(numRecords, 256)), B, args);
    LAUNCH(ctx, "kernel.intersect.report", reportKernel, dim3(std::min(divUp(nt, 256), LOOP_BLOCKS)), B, (const uint32_t *) dPartners, nt,
           counters.get());
    LAUNCH(ctx, "kernel.intersect.report", mostKernel, dim3(divUp(nt, 256)), B, (const uint32_t *) dPartners, nt, counters.get());
    PROPAGATE(counters.readBack(ctx));
    out->candidatePairs = h[C_CANDIDATES];
    out->crossingPairs = h[C_CROSSINGS];
    out->crossingTriangles = h[C_CROSSING_TRIANGLES];
    out->maxPartners = h[C_MAX_PARTNERS];
    if (out->crossingPairs > 0)
    {
        out->lowestA = h[C_LOWEST] >> 32;
        out->lowestB = h[C_LOWEST] & 0xFFFFFFFFu;
        out->maxPartnersTriangle = h[C_MAX_TRIANGLE];
    }
    if (ctx->timing)
        ctx->addValue("intersect.pairs.tested", (double) h[C_TESTED]);

    /* the list, where it is taken and fits: the walk once more over the triangles that have a partner, the crossing pairs
     * appended in whatever order the lanes arrive, and a sort that makes the order the contract's */
    const uint64_t numPairs = out->crossingPairs;
    if (dPairs != nullptr && pairCapacity < numPairs)
    {
        if (ctx->timing)
            ctx->addValue("intersect.scratch.bytes", scratch);
        return setError(MLSGPU_ERR_LENGTH, "mesh self-intersections: %llu crossing pairs, room for %llu", (unsigned long long) numPairs,
                        (unsigned long long) pairCapacity);
    }
    if (dPairs != nullptr && numPairs > 0)
    {
        REQUIRE(numPairs < (uint64_t(1) << 32), MLSGPU_ERR_LENGTH);
        PROPAGATE(found.alloc(numPairs));
        scratch += (double) found.bytes();
        args.list = found.keys();
        args.listCapacity = numPairs;
        LAUNCH(ctx, "kernel.intersect.list", (pairsKernel<true>), dim3(divUp(numRecords, 256)), B, args);
        /* (both sorts under one name: a launch site of the sort keeps one stat id per translation unit) */
        SortResult<uint64_t> sorted = {nullptr, nullptr};
        PROPAGATE(radixSort<uint64_t>(ctx, "kernel.intersect.sort", found.keysA, found.valsA, found.keysB, found.valsB, numPairs,
                                      32 + bitLength(nt - 1), true, found.hist, nullptr, &sorted));
        LAUNCH(ctx, "kernel.intersect.list", unpackKernel, dim3(divUp(numPairs, 256)), B, (const uint64_t *) sorted.keys, numPairs, dPairs);
        PROPAGATE(counters.readBack(ctx));
        if (h[C_CURSOR] != numPairs)
            return setError(MLSGPU_ERR_HIP, "mesh self-intersections: the list pass found %llu pairs, the count %llu", h[C_CURSOR],
                            (unsigned long long) numPairs);
    }
    if (ctx->timing)
        ctx->addValue("intersect.scratch.bytes", scratch);
    return MLSGPU_OK;
}
