/*
 * Splat octree build on gfx950 -- the device half of SplatTreeCL
 * (reference: src/splat_tree_cl.{h,cpp}, kernels/octree.cl).
 *
 * Output contract (identical to the reference, checked bit-for-bit against the oracle):
 * `start` (one int per node, levels stored finest first) and `commands`
 * ([end][ids...][jump] per non-empty node), see src/splat_tree.h:40-74.
 *
 * Differences in mechanism (not in results):
 *  - the indicator (countCommands) and commandMap arrays are never materialised: the indicator
 *    is recomputed from the sorted keys inside the scan, and writeSplatIds is the scan's consumer;
 *  - the per-level writeStart launches (levels dependent launches in the reference) are one
 *    launch: every node finds its nearest non-empty strict ancestor by itself;
 *  - the sort handles 3*(maxShift-minShift)+1 key bits in ceil(bits/10) stable passes.
 */
#include "common.hpp"
#include "primitives.hpp"

#include <cstdlib>

using namespace mlsgpu;

struct LevelOffsets
{
    uint32_t v[32];
};

struct mlsgpu_tree
{
    mlsgpu_ctx *ctx = nullptr;
    uint64_t maxLevels = 0, maxSplats = 0;
    uint64_t maxStart = 0, commandsSize = 0;
    uint32_t numLevels = 0;
    DeviceArray<int32_t> dStart, dJumpPos, dCommands;
    DeviceArray<uint32_t> dKeysA, dKeysB, dValsA, dValsB;
    DeviceArray<uint32_t> dHist, dTileSums, dNumEntries;
    DeviceArray<uint32_t> dNodeCounts, dNodeBase;   /* per node: entries, and twice the non-empty nodes before it */
    DeviceArray<uint32_t> dDigitBase;   /* 257 words: where the groups of the fused first pass begin (packed entries) */
    DeviceArray<U3> dNodeTiles;         /* tile sums of the scan over the nodes */
    HostMailbox entryBox;               /* the entry count comes back to the host once per build */
    DeviceArray<uint8_t> dSlotMasks;    /* per splat: which of its 8 candidate slots are real entries */
    DeviceArray<uint64_t> dEntryNotes;  /* per splat, the fused front end: slot mask, level, node coordinates (packNote) */
    mlsgpu_splat *dSplats = nullptr;   /* borrowed between build and clear_splats */
    bool mutate = true;                 /* radius -> 1/radius^2 in place (the reference); false: the splats stay as they came */

    mlsgpu_tree(uint64_t maxLevels, uint64_t maxSplats) : maxLevels(maxLevels), maxSplats(maxSplats)
    {
        /* src/splat_tree_cl.cpp:112-123 */
        maxStart = (uint64_t(1) << (3 * maxLevels)) / 7;
        commandsSize = maxSplats * 8 + std::min(maxStart, 8 * maxSplats) * 2;
    }
    ~mlsgpu_tree() { entryBox.destroy(); }

    /* Every device buffer of the tree with its element count, once: each(array, elements) until one fails.
     * mlsgpu_hip_tree_create allocates them, mlsgpu_hip_tree_resource_usage adds them up. */
    template<typename Each>
    int buffers(Each each)
    {
        const uint64_t entries = maxSplats * 8;
        const uint64_t histElems = sortHistElems(entries);
        PROPAGATE(each(dStart, maxStart));
        PROPAGATE(each(dJumpPos, maxStart));
        PROPAGATE(each(dCommands, commandsSize));
        PROPAGATE(each(dKeysA, entries));
        PROPAGATE(each(dKeysB, entries));
        PROPAGATE(each(dValsA, entries));
        PROPAGATE(each(dValsB, entries));
        PROPAGATE(each(dHist, histElems));
        PROPAGATE(each(dTileSums, (uint64_t) scanTiles(std::max(histElems, entries)) + 1));
        PROPAGATE(each(dNumEntries, 1));
        PROPAGATE(each(dSlotMasks, maxSplats));
        PROPAGATE(each(dEntryNotes, maxSplats));
        PROPAGATE(each(dNodeCounts, maxStart));
        PROPAGATE(each(dNodeBase, maxStart));
        PROPAGATE(each(dDigitBase, 257));
        PROPAGATE(each(dNodeTiles, (uint64_t) scanTiles(maxStart) + 1));
        return MLSGPU_OK;
    }
};

namespace
{

/* kernels/octree.cl:121-136 (z-major Morton); coordinates here are < 2^10 */
__device__ __forceinline__ uint32_t spread3(uint32_t v)
{
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
/* spread3(v + 1) from spread3(v): with the gaps between the coordinate's bits filled the carry runs through them
 * (1023 + 1 gives 0, as the mask of spread3 does) */
__device__ __forceinline__ uint32_t spreadNext(uint32_t s)
{
    return ((s | ~0x09249249u) + 1u) & 0x09249249u;
}
/* Bit b of x, y, z goes to bit 3b, 3b + 1, 3b + 2: the low three bits of a code are the PARITIES of its coordinates.
 * entryScatterKernel's ranking rests on that (mls.hip's spread3 interleaves the same way). */
__device__ __forceinline__ uint32_t makeCode(int x, int y, int z)
{
    return spread3((uint32_t) x) | (spread3((uint32_t) y) << 1) | (spread3((uint32_t) z) << 2);
}
static_assert((0x09249249u & 7u) == 1u, "spread3 keeps bit 0 of a coordinate in bit 0");

/* general form for the test kernel (any non-negative ints), octree.cl:121-136 verbatim semantics */
__device__ uint32_t makeCodeLoop(int x, int y, int z)
{
    uint32_t ans = 0, scale = 1;
    y <<= 1;
    z <<= 2;
    while (x != 0 || y != 0 || z != 0)
    {
        uint32_t bits = (x & 1) | (y & 2) | (z & 4);
        ans += bits * scale;
        scale <<= 3;
        x >>= 1; y >>= 1; z >>= 1;
    }
    return ans;
}

/* kernels/octree.cl:50-55 */
__device__ __forceinline__ int levelShift(int lox, int loy, int loz, int hix, int hiy, int hiz)
{
    int big = max(max(hix - lox, hiy - loy), hiz - loz);
    return big > 1 ? 32 - __clz(big - 1) : 0;
}

/* kernels/octree.cl:60-66: OpenCL dot() restated as a plain sum of products (no fma) */
__device__ __forceinline__ float pointBoxDist2(float px, float py, float pz, float lx, float ly, float lz,
                                                float hx, float hy, float hz)
{
    float dx = fmaxf(lx, fminf(hx, px)) - px;
    float dy = fmaxf(ly, fminf(hy, py)) - py;
    float dz = fmaxf(lz, fminf(hz, pz)) - pz;
    return dx * dx + dy * dy + dz * dz;
}

/* convert_int_rtn: floor then saturating convert (v_cvt_i32_f32 saturates) */
__device__ __forceinline__ int floorToInt(float v)
{
    float f = floorf(v);
    if (!(f > -2147483648.0f)) return INT32_MIN;
    if (!(f < 2147483648.0f)) return INT32_MAX;
    return (int) f;
}

/* The per-splat part of writeEntries, kernels/octree.cl:159-214 (+prepare :79-90, goodEntry :100-110):
 * the up-to-8 sort keys of one splat; returns the bit mask of the slots that hold a real entry
 * (the reference writes UINT_MAX into the others). */
struct EntryParams
{
    mlsgpu_splat *splats;
    int bx, by, bz;
    LevelOffsets levelOffsets;
    int minShift, maxShift;
    uint32_t firstSplat;
    uint32_t mutate;            /* write 1/r^2 into the radius slot (kernels/octree.cl:193), or leave the splats untouched */
};

/* ... and where its 2 x 2 x 2 candidate nodes are: level and lowest node coordinates (what a key is made of) */
struct EntryPlace
{
    int shift, ilx, ily, ilz;
};

__device__ __forceinline__ uint32_t splatEntries(const EntryParams &P, const float4 pr, uint32_t k[8], EntryPlace *place = nullptr)
{
    /* prepare, octree.cl:79-90 */
    const int lox = floorToInt(pr.x - pr.w), loy = floorToInt(pr.y - pr.w), loz = floorToInt(pr.z - pr.w);
    const int hix = floorToInt(pr.x + pr.w), hiy = floorToInt(pr.y + pr.w), hiz = floorToInt(pr.z + pr.w);
    int shift = levelShift(lox, loy, loz, hix, hiy, hiz);
    shift = min(max(shift, P.minShift), P.maxShift);
    const int ilx = max(lox - P.bx, 0) >> shift;
    const int ily = max(loy - P.by, 0) >> shift;
    const int ilz = max(loz - P.bz, 0) >> shift;
    float radius2 = pr.w * pr.w;
    radius2 *= 1.00001f;
    const uint32_t levelOffset = P.levelOffsets.v[shift];
    const int bound = 1 << (P.maxShift - shift);
    if (place != nullptr)
        *place = EntryPlace{shift, ilx, ily, ilz};
    uint32_t mask = 0;
#pragma unroll
    for (int o = 0; o < 8; o++)
    {
        const int ax = ilx + (o & 1), ay = ily + ((o >> 1) & 1), az = ilz + (o >> 2);
        /* goodEntry, octree.cl:100-110; int arithmetic wraps like OpenCL's */
        const int blx = (int) ((uint32_t) ax << shift) + P.bx, bhx = (int) ((uint32_t) (ax + 1) << shift) + P.bx;
        const int bly = (int) ((uint32_t) ay << shift) + P.by, bhy = (int) ((uint32_t) (ay + 1) << shift) + P.by;
        const int blz = (int) ((uint32_t) az << shift) + P.bz, bhz = (int) ((uint32_t) (az + 1) << shift) + P.bz;
        bool isect = pointBoxDist2(pr.x, pr.y, pr.z, (float) blx, (float) bly, (float) blz,
                                   (float) bhx, (float) bhy, (float) bhz) < radius2;
        isect = isect && ax < bound && ay < bound && az < bound;
        /* inside the bounds the coordinates fit 10 bits (maxShift - shift <= 9 levels) */
        k[o] = makeCode(ax, ay, az) + levelOffset;
        mask |= (isect ? 1u : 0u) << o;
    }
    return mask;
}

/*
 * writeEntries as a compaction: the reference writes 8 (key, id) slots per splat and lets the UINT_MAX
 * ones sort to the end, where writeSplatIds ignores them (kernels/octree.cl:263).  Here only the real
 * entries are written, densely, in the same (splat, slot) order -- a stable sort of the survivors gives
 * exactly the order the padded array would have had before its UINT_MAX tail, so `commands` and `start`
 * are unchanged while sort, scan and writeSplatIds touch about half the data.
 * Producer: number of real entries of splat i.  Consumer: writes them at the scanned position and
 * replaces splat.w by 1/r^2 (:193).
 */
struct EntryCountIn            /* phase 1: evaluates the splat, remembers which slots are real entries */
{
    EntryParams P;
    uint8_t *slotMasks;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        const float4 pr = reinterpret_cast<const float4 *>(P.splats + (i + P.firstSplat))[0];
        uint32_t k[8];
        const uint32_t mask = splatEntries(P, pr, k);
        slotMasks[i] = (uint8_t) mask;
        return (uint32_t) __popc(mask);
    }
};

struct EntryMaskIn             /* phase 2: the count again, from the remembered mask */
{
    const uint8_t *slotMasks;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const { return (uint32_t) __popc((uint32_t) slotMasks[i]); }
};

struct EntryWriteOut
{
    EntryParams P;
    const uint8_t *slotMasks;
    uint32_t *keys, *values;
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t pos, uint32_t) const
    {
        const uint32_t gid = (uint32_t) i + P.firstSplat;
        float4 *sp = reinterpret_cast<float4 *>(P.splats + gid);
        const float4 pr = sp[0];
        if (P.mutate)
            reinterpret_cast<float *>(sp)[3] = 1.0f / (pr.w * pr.w);
        const uint32_t mask = slotMasks[i];
        if (mask == 0)
            return;
        /* prepare (octree.cl:79-90) again for the node coordinates; the box tests are not repeated */
        const int lox = floorToInt(pr.x - pr.w), loy = floorToInt(pr.y - pr.w), loz = floorToInt(pr.z - pr.w);
        const int hix = floorToInt(pr.x + pr.w), hiy = floorToInt(pr.y + pr.w), hiz = floorToInt(pr.z + pr.w);
        int shift = levelShift(lox, loy, loz, hix, hiy, hiz);
        shift = min(max(shift, P.minShift), P.maxShift);
        const int ilx = max(lox - P.bx, 0) >> shift;
        const int ily = max(loy - P.by, 0) >> shift;
        const int ilz = max(loz - P.bz, 0) >> shift;
        const uint32_t levelOffset = P.levelOffsets.v[shift];
#pragma unroll
        for (int o = 0; o < 8; o++)
            if (mask & (1u << o))
            {
                keys[pos] = makeCode(ilx + (o & 1), ily + ((o >> 1) & 1), ilz + (o >> 2)) + levelOffset;
                values[pos] = gid;
                pos++;
            }
    }
};

/*
 * writeEntries fused with the FIRST pass of the entry sort (round 3).  The entries of a tile of ENT_TILE splats are never
 * written in (splat, slot) order: the counting kernel histograms the low digit of their keys per tile while it evaluates the
 * box tests, one digit scan turns the histograms into positions (the same kernel the sort uses), and the scattering kernel
 * regenerates the tile's entries from the remembered notes, ranks them as a stable sort that starts from (splat, slot)
 * order would (see entryScatterKernel) and sends them straight to where the first LSD pass would have put them.  That is one
 * write and one read of all entries (16 bytes each) and two launches less than writeEntries + histogram + scatter; the
 * remaining passes of the sort are unchanged.  Results are identical: same keys, same stable order.
 */
enum
{
    ENT_THREADS = 512,              /* threads per workgroup */
    ENT_PER = 2,                    /* splats per thread (1 or 2).  entryHist + entryScatter per launch of four buckets
                                     * (cfg3): 1 splat per thread 93.6 + 75.6 us, 2: 96.3 + 69.4 -- twice as long a run of
                                     * every digit in memory, and three workgroups still fit a CU's LDS
                                     * (profiles/NOTES_entry_rank.md) */
    ENT_TILE = ENT_THREADS * ENT_PER,   /* splats per workgroup */
    ENT_CAP = 8 * ENT_TILE,         /* at most eight entries per splat */
    ENT_BIN_BITS = 8,               /* the fused pass handles digits of up to 8 bits */
    ENT_KEY_BITS = 22,              /* ... of keys that leave ten bits of a word for the splat's place in the tile */
    ENT_MIN_DIGIT_BITS = 3          /* ... and of at least 3, or of a one-level tree: see entryScatterKernel */
};
static_assert(ENT_PER == 1 || ENT_PER == 2, "the splat's place in the tile has 32 - ENT_KEY_BITS bits");

/* What entryHist leaves entryScatter per splat, 8 bytes: low word = slot mask (bits 0-7), level (8-12), lowest node x
 * (13-22); high word = lowest node y (0-9) and z (10-19); ten bits per coordinate inside the bounds -- so the scatter reads
 * 8 bytes per splat instead of the 32-byte record (of which it needed 16) and repeats none of the arithmetic.  0 = no entry. */
__device__ __forceinline__ uint64_t packNote(uint32_t mask, const EntryPlace &pl)
{
    if (mask == 0)
        return 0;
    const uint32_t lo = mask | (uint32_t) pl.shift << 8 | ((uint32_t) pl.ilx & 0x3FFu) << 13;
    const uint32_t hi = ((uint32_t) pl.ily & 0x3FFu) | ((uint32_t) pl.ilz & 0x3FFu) << 10;
    return (uint64_t) lo | (uint64_t) hi << 32;
}

struct EntryHistArgs
{
    EntryParams P;
    uint64_t *notes;
    uint32_t *hist;
    uint32_t numTiles;
    uint64_t n;
};

__global__ __launch_bounds__(ENT_THREADS) void entryHistKernel(Lanes<EntryHistArgs> lanes, uint32_t digitBits)
{
    const EntryHistArgs &A = lanes.a[blockIdx.y];     /* by reference: the level offsets are indexed dynamically and stay
                                                         * in the kernel-argument segment (a copy would live in scratch) */
    if (blockIdx.x >= A.numTiles)
        return;
    __shared__ uint32_t bins[1 << ENT_BIN_BITS];
    const uint32_t numBins = 1u << digitBits, dmask = numBins - 1;
    for (uint32_t d = threadIdx.x; d < numBins; d += ENT_THREADS)
        bins[d] = 0;
    __syncthreads();
    /* a thread's splats are neighbours in the cloud (one 32 x ENT_PER-byte stretch): both records are requested before the
     * first is looked at */
    const uint32_t tile = tileOfWorkgroup(blockIdx.x, A.numTiles);      /* its counters' lines are completed in one XCD's L2 */
    const uint64_t i0 = (uint64_t) tile * ENT_TILE + (uint64_t) threadIdx.x * ENT_PER;
    float4 pr[ENT_PER];
#pragma unroll
    for (int s_ = 0; s_ < ENT_PER; s_++)
        pr[s_] = reinterpret_cast<const float4 *>(A.P.splats + ((i0 + s_ < A.n ? i0 + s_ : 0) + A.P.firstSplat))[0];
#pragma unroll
    for (int s_ = 0; s_ < ENT_PER; s_++)
        if (i0 + s_ < A.n)
        {
            uint32_t k[8];
            EntryPlace pl;
            const uint32_t mask = splatEntries(A.P, pr[s_], k, &pl);
            A.notes[i0 + s_] = packNote(mask, pl);
            if (A.P.mutate)     /* kernels/octree.cl:193; nothing behind this kernel reads the radius */
                reinterpret_cast<float *>(A.P.splats + ((i0 + s_) + A.P.firstSplat))[3] = 1.0f / (pr[s_].w * pr[s_].w);
#pragma unroll
            for (int o = 0; o < 8; o++)
                if (mask & (1u << o))
                    atomicAdd(&bins[k[o] & dmask], 1u);
        }
    __syncthreads();
    uint32_t *const hist = A.hist;
    const uint32_t numTiles = A.numTiles;
    for (uint32_t d = threadIdx.x; d < numBins; d += ENT_THREADS)
        hist[(uint64_t) d * numTiles + tile] = bins[d];
}

struct EntryTotalArgs
{
    const uint32_t *digitTotals;
    uint32_t *total;
    uint32_t *digitBase;        /* [numBins + 1]: exclusive prefix of the totals -- where every digit's group begins */
};

/* the number of entries = the sum of the digit totals; one workgroup adds up every lane's in turn */
__global__ __launch_bounds__(256) void entryTotalKernel(Lanes<EntryTotalArgs> lanes, uint32_t count, uint32_t numBins,
                                                        uint32_t *box, uint32_t seq)
{
    __shared__ uint32_t waveTotals[4];
    for (uint32_t k = 0; k < count; k++)
    {
        const uint32_t *const digitTotals = lanes.a[k].digitTotals;
        /* numBins <= 256 (ENT_BIN_BITS): one digit per thread */
        const uint32_t mine = threadIdx.x < numBins ? digitTotals[threadIdx.x] : 0u;
        const uint32_t incl = waveInclusiveScan(mine);
        if ((threadIdx.x & 63) == 63)
            waveTotals[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t before = 0;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++)
            before += waveTotals[w];
        if (threadIdx.x < numBins)
            lanes.a[k].digitBase[threadIdx.x] = before + incl - mine;
        if (threadIdx.x == 0)
        {
            const uint32_t sum = waveTotals[0] + waveTotals[1] + waveTotals[2] + waveTotals[3];
            lanes.a[k].digitBase[numBins] = sum;
            *lanes.a[k].total = sum;
            /* ... and straight to the host (HostMailbox): the count sizes the launches that follow */
            __hip_atomic_store(box + 1 + k, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0)
    {
        __threadfence_system();
        __hip_atomic_store(box, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

struct EntryScatterArgs
{
    EntryParams P;
    const uint64_t *notes;
    const uint32_t *hist;
    const uint32_t *digitTotals;
    uint32_t numTiles;
    uint64_t n;
    uint32_t *keysOut, *valsOut;
    uint32_t idBits;            /* != 0: an entry leaves as ONE word, (key >> digitBits) << idBits | (id - firstSplat), in keysOut */
};

/* The keys of one splat's 2 x 2 x 2 candidate nodes, from its note, times 8 (the bytes of a matrix word, see
 * entryScatterKernel).  Morton digits are independent, so the spread coordinates have no bit in common and makeCode of
 * the node (ilx + dx, ily + dy, ilz + dz) is a SUM of one part per axis: a key is one addition of two of six values that
 * are made once per splat -- the kernel issues vector instructions for all eight slots of its splats, full or not, and is
 * bound by their number. */
struct NoteKeys
{
    uint32_t x[2], yz[4];
    NoteKeys() = default;
    __device__ __forceinline__ NoteKeys(uint64_t note, const LevelOffsets &levelOffsets)
    {
        const uint32_t lo32 = (uint32_t) note, hi32 = (uint32_t) (note >> 32);
        const uint32_t ilx = (lo32 >> 13) & 0x3FFu, ily = hi32 & 0x3FFu, ilz = (hi32 >> 10) & 0x3FFu;
        const uint32_t levelOffset = levelOffsets.v[(lo32 >> 8) & 0x1Fu];      /* (a note of 0: level 0, never used) */
        const uint32_t sx[2] = {spread3(ilx), spreadNext(spread3(ilx))};
        const uint32_t sy[2] = {spread3(ily), spreadNext(spread3(ily))};
        const uint32_t sz[2] = {spread3(ilz), spreadNext(spread3(ilz))};
        for (uint32_t i = 0; i < 2; i++)
            x[i] = sx[i] << 3;
        for (uint32_t i = 0; i < 4; i++)
            yz[i] = (sy[i & 1] << 4) + (sz[i >> 1] << 5) + (levelOffset << 3);
    }
    /* == 8 * (makeCode(ilx + (o & 1), ily + ((o >> 1) & 1), ilz + (o >> 2)) + levelOffset) */
    __device__ __forceinline__ uint32_t key8(int o) const { return x[o & 1] + yz[o >> 1]; }
};

/*
 * How the tile's entries are ranked.  The pass is one stable split of the tile's entries, taken in (splat, slot) order, by
 * the low digit of their keys.  A generic split has to order the entries first and rank them round by round; this one
 * does not, because NO TWO ENTRIES OF A SPLAT SHARE A DIGIT:
 *  - a splat's entries are among the eight nodes (ilx + dx, ily + dy, ilz + dz), dx, dy, dz in {0, 1}, of ONE level, all
 *    inside the bounds (goodEntry), where every coordinate is below 2^10;
 *  - makeCode puts the lowest bit of x, y and z into bits 0, 1 and 2 of the code (spread3: bit b of a coordinate goes to
 *    bit 3b, and y and z are shifted by 1 and 2) -- the parities of the coordinates.  ilx and ilx + 1 differ in parity
 *    whatever carries the addition causes above bit 0, so the eight codes differ pairwise in their low three bits;
 *  - all eight get the one levelOffset added, which permutes the residues modulo 8: the keys stay distinct modulo 8,
 *    hence modulo every 2^b with b >= 3 (ENT_MIN_DIGIT_BITS).
 * A narrower digit reaches this kernel only from a tree of ONE level (treeBuildBatch), where bound = 1 leaves a splat its
 * slot 0 at most: one entry, nothing to share.
 * So the stable rank of an entry among the tile's entries with its digit is the number of EARLIER SPLATS of the tile that
 * hold that digit: with one bit per (digit, splat) in LDS -- match[group][digit], bit l = splat 64 * group + l of the
 * tile -- that is a count of words before the splat's group plus a population count below its bit.  Every slot's
 * operations are independent of every other slot's; nothing goes round by round.
 */
__global__ __launch_bounds__(ENT_THREADS) __attribute__((amdgpu_waves_per_eu(ENT_PER == 2 ? 6 : 8, 8))) void entryScatterKernel(Lanes<EntryScatterArgs> lanes, uint32_t digitBits)
{
    enum { BINS = 1 << ENT_BIN_BITS, WAVES = ENT_THREADS / 64, GROUPS = ENT_TILE / 64, MAX_ROUNDS = ENT_CAP / ENT_THREADS };
    static_assert(BINS <= ENT_THREADS, "one thread per bin in the scan over the digits");
    const EntryScatterArgs &A = lanes.a[blockIdx.y];  /* by reference, as in entryHistKernel */
    if (blockIdx.x >= A.numTiles)
        return;
    const EntryParams &P = A.P;
    const uint64_t *const notes = A.notes;
    const uint32_t *const hist = A.hist;
    const uint32_t *const digitTotals = A.digitTotals;
    const uint32_t numTiles = A.numTiles;
    const uint64_t n = A.n;
    uint32_t *const keysOut = A.keysOut, *const valsOut = A.valsOut;
    /* The matrix is dead once every entry knows its place, and the entries are lined up only then: both live in the same
     * 32 KB, the matrix of the WHOLE tile (no second half through a re-zeroed one).  An entry in LDS is ONE word: its key
     * (ENT_KEY_BITS at most on this route) below its splat's place in the tile (the id is the tile's first id + that).
     * With sPlace 49 KB for a tile of 1024 splats: three workgroups per CU. */
    typedef unsigned long long Word;
    __shared__ union
    {
        Word match[GROUPS][BINS];               /* conflict-free over the digits; a group's words belong to ONE wave */
        uint32_t ent[ENT_CAP];                  /* the tile's entries in the pass's order */
    } s;
    static_assert(sizeof(s.match) <= sizeof(s.ent), "the matrix fits the entries' space");
    __shared__ uint32_t sPlace[GROUPS][BINS];   /* per group and digit: where the group's first entry with the digit goes in
                                                 * the tile; half a matrix word's offset is this table's */
    __shared__ uint32_t tileBase[BINS];         /* what takes a place in the tile to its place in memory */
    __shared__ uint32_t waveTotals[WAVES], waveTotalsAll[WAVES];
    const uint32_t numBins = 1u << digitBits, dmask = numBins - 1;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < GROUPS * BINS; i += ENT_THREADS)
        (&s.match[0][0])[i] = 0ull;
    /* 1. one bit per entry.  Thread t holds splats t, t + ENT_THREADS (, ...) of the tile: a wave's 64 notes are one 512-byte
     * stretch, and a wave's splats are one group of the matrix per round -- lane l is bit l.  What the thread reads that
     * does not depend on another read is requested here, together: its notes, and the digit total and tile offset of the
     * bin it owns in the scan further down. */
    const uint32_t tile = tileOfWorkgroup(blockIdx.x, numTiles);
    uint64_t note[ENT_PER];
#pragma unroll
    for (int h = 0; h < ENT_PER; h++)
    {
        const uint64_t i = (uint64_t) tile * ENT_TILE + (uint32_t) h * ENT_THREADS + threadIdx.x;
        note[h] = i < n ? notes[i] : 0ull;
    }
    const uint32_t bin = threadIdx.x;
    const uint32_t totalOfBin = bin < numBins ? digitTotals[bin] : 0u;
    const uint32_t histOfBin = bin < numBins ? hist[(uint64_t) bin * numTiles + tile] : 0u;
    NoteKeys keys[ENT_PER];
#pragma unroll
    for (int h = 0; h < ENT_PER; h++)
        keys[h] = NoteKeys(note[h], P.levelOffsets);
    /* the matrix word of slot o of splat h, as a byte offset: the row of the splat's group | 8 * the key's digit */
    const uint32_t dmask8 = dmask << 3;
    auto wordOf = [&](int h, int o) { return (keys[h].key8(o) & dmask8) | (((uint32_t) h * WAVES + wave) * (uint32_t) sizeof(s.match[0])); };
    auto matchAt = [&](uint32_t w) { return reinterpret_cast<Word *>(reinterpret_cast<char *>(&s.match[0][0]) + w); };
    auto placeAt = [&](uint32_t w) { return reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(&sPlace[0][0]) + (w >> 1)); };
    __syncthreads();
    const Word bit = 1ull << lane;
#pragma unroll
    for (int h = 0; h < ENT_PER; h++)
#pragma unroll
        for (int o = 0; o < 8; o++)
            if (note[h] & (1u << o))
                atomicOr(matchAt(wordOf(h, o)), bit);       /* nothing comes back */
    __syncthreads();
    /* 2. per digit, the counts of its words and their exclusive prefix along the groups; the sum is the tile's histogram
     * entry.  Then the scan over the bins: where the digit's run begins in the tile, and in memory. */
    uint32_t mine = 0, before[GROUPS];
    if (bin < numBins)
    {
#pragma unroll
        for (int g = 0; g < GROUPS; g++)
        {
            before[g] = mine;
            mine += (uint32_t) __popcll(s.match[g][bin]);
        }
    }
    {
        const uint32_t inclMine = waveInclusiveScan(mine), inclAll = waveInclusiveScan(totalOfBin);
        if (lane == 63)
        {
            waveTotals[wave] = inclMine;
            waveTotalsAll[wave] = inclAll;
        }
        __syncthreads();
        uint32_t run = inclMine - mine, base = inclAll - totalOfBin;
        for (uint32_t w = 0; w < wave; w++)
        {
            run += waveTotals[w];
            base += waveTotalsAll[w];
        }
        if (bin < numBins)
        {
#pragma unroll
            for (int g = 0; g < GROUPS; g++)
                sPlace[g][bin] = run + before[g];
            tileBase[bin] = base + histOfBin - run;
        }
    }
    uint32_t tileCount = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++)
        tileCount += waveTotals[w];
    if (tileCount == 0)
        return;
    __syncthreads();
    /* every entry's place in the pass's order: its group's first + the splats below its own in the word (the last reads
     * of the matrix) */
    uint32_t dst[ENT_PER][8];
#pragma unroll
    for (int h = 0; h < ENT_PER; h++)
#pragma unroll
        for (int o = 0; o < 8; o++)
            if (note[h] & (1u << o))
            {
                const uint32_t w = wordOf(h, o);
                const Word m = *matchAt(w);
                dst[h][o] = __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, *placeAt(w)));
            }
    __syncthreads();
    /* ... and the entries go there, over the matrix */
#pragma unroll
    for (int h = 0; h < ENT_PER; h++)
    {
        const uint32_t holder = ((uint32_t) h * ENT_THREADS + threadIdx.x) << ENT_KEY_BITS;
#pragma unroll
        for (int o = 0; o < 8; o++)
            if (note[h] & (1u << o))
                s.ent[dst[h][o]] = (keys[h].key8(o) >> 3) | holder;
    }
    __syncthreads();
    /* 3. out, in the order of the pass: the run of a digit is contiguous in the tile and in memory */
    const uint32_t idBits = A.idBits;
    const uint32_t tileFirstId = tile * ENT_TILE + (idBits != 0 ? 0u : P.firstSplat);
#pragma unroll
    for (int k = 0; k < MAX_ROUNDS; k++)
    {
        const uint32_t p = threadIdx.x + k * ENT_THREADS;
        if (p < tileCount)
        {
            const uint32_t e = s.ent[p];
            const uint32_t key = e & ((1u << ENT_KEY_BITS) - 1u);
            const uint32_t out = tileBase[key & dmask] + p;
            const uint32_t id = tileFirstId + (e >> ENT_KEY_BITS);
            if (idBits != 0)
                keysOut[out] = (key >> digitBits) << idBits | id;     /* the digit is where the entry lies from now on */
            else
            {
                keysOut[out] = key;
                valsOut[out] = id;
            }
        }
    }
}

/*
 * The last pass of the entry sort on the packed route (one word per entry, top digit << idBits | id; the key's low part is
 * the group of the fused pass the word lies in, group g at [lowBase[g], lowBase[g + 1])): commandHistKernel counts the top
 * digits per tile and the whole keys, commandScatterKernel sends every id to its command position.  They compute what
 * sortHistKernel<uint32_t, true> and sortScatterKernel<uint32_t, false, 8, true> compute on these words (primitives.hpp;
 * MLSGPU_HIP_OCTREE_LAST_PASS=0 takes those, for A/B) -- same tiles, same [digit][tile] histogram, same order -- with the
 * work a tile of packed words does not need left out: a tile is FULL (every one but a lane's last) and lies in ONE low part
 * (six of seven on the headline cloud) or it does not, which the workgroup finds out once, and the common tile runs
 * straight-line code.  Digits have 8 bits at most here (the fused pass's limit), so a thread owns one bin.
 */
enum { CMD_BINS = 1 << ENT_BIN_BITS };
static_assert(CMD_BINS == PRIM_BLOCK, "one bin and one group begin per thread");

/* The groups the tile's first and last element lie in: counts of group begins at or before them (group 0 begins at 0; an
 * empty group begins where the next one does, so the count lands on the group that holds the position).  Every wave counts
 * all numLow <= 256 begins itself: nothing crosses waves, nothing waits for a barrier.  myBegin: lowBase[threadIdx.x]. */
__device__ __forceinline__ void lowPartsOfTile(const uint32_t *lowBase, uint32_t numLow, uint32_t first, uint32_t last,
                                               uint32_t &lowFirst, bool &oneLow, uint32_t &myBegin)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    /* lowBase has CMD_BINS + 1 words whatever numLow is (dDigitBase): all four are requested before the first is looked at */
    uint32_t begins[PRIM_WAVES];
#pragma unroll
    for (uint32_t q = 0; q < PRIM_WAVES; q++)
        begins[q] = lowBase[q * 64 + lane];
    uint32_t c0 = 0, c1 = 0;
    myBegin = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t q = 0; q < PRIM_WAVES; q++)
    {
        const uint32_t begin = q * 64 + lane < numLow ? begins[q] : 0xFFFFFFFFu;
        c0 += (uint32_t) __popcll(__ballot(begin <= first));
        c1 += (uint32_t) __popcll(__ballot(begin <= last));
        if (q == wave)
            myBegin = begin;
    }
    lowFirst = c0 - 1;
    oneLow = c1 == c0;
}

struct CommandHistArgs
{
    const uint32_t *words;
    uint32_t *hist;
    uint32_t n;
    const uint32_t *nDev;
    uint32_t numTiles;
    uint32_t *keyCounts;        /* occurrences of every whole key, (top digit << shift) | low part */
    const uint32_t *lowBase;    /* CMD_BINS + 1 words, the first 2^shift + 1 of them written */
};

__global__ __launch_bounds__(PRIM_BLOCK) void commandHistKernel(Lanes<CommandHistArgs> lanes, uint32_t shift, uint32_t digitBits,
                                                                uint32_t idBits)
{
    const CommandHistArgs A = lanes.a[blockIdx.y];
    if (blockIdx.x >= A.numTiles)
        return;
    uint32_t n = A.n;
    if (A.nDev != nullptr && *A.nDev < n)
        n = *A.nDev;
    __shared__ uint32_t bins[CMD_BINS];
    __shared__ uint32_t keyBins[KEY_COUNT_SLOTS * CMD_BINS];
    __shared__ uint32_t sLow[CMD_BINS];
    const uint32_t numBins = 1u << digitBits, numLow = 1u << shift;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t tile = tileOfWorkgroup(blockIdx.x, A.numTiles);
    const uint32_t tileFirst = tile * SORT_TILE;
    /* (0: a tile behind nDev still reports its histogram, all zeros) */
    const uint32_t tileCount = tileFirst >= n ? 0u : n - tileFirst < SORT_TILE ? n - tileFirst : (uint32_t) SORT_TILE;
    const bool full = tileCount == SORT_TILE;
    const uint32_t at = wave * SORT_WAVE_SPAN + lane;           /* the thread's first element in the tile */
    const uint32_t *const words = A.words + tileFirst + at;
    /* all of the thread's words are requested before the first is counted, and the group begins with them */
    uint32_t mine[SORT_ITEMS];
    if (full)
    {
        /* (four words to a load, a wave's load one KB, was measured and changed nothing: 40.9 against 40.2 us) */
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            mine[j] = words[j * 64];
    }
    else
    {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            mine[j] = at + j * 64 < tileCount ? words[j * 64] : 0u;
    }
    uint32_t lowFirst = 0, myBegin;
    bool oneLow = true;
    lowPartsOfTile(A.lowBase, numLow, tileFirst, tileFirst + (tileCount != 0 ? tileCount - 1 : 0u), lowFirst, oneLow, myBegin);
    bins[threadIdx.x] = 0;
    if (!oneLow)        /* (uniform over the workgroup) */
    {
        sLow[threadIdx.x] = myBegin;
#pragma unroll
        for (uint32_t d = threadIdx.x; d < KEY_COUNT_SLOTS * CMD_BINS; d += PRIM_BLOCK)
            keyBins[d] = 0;
    }
    __syncthreads();
    if (full && oneLow)
    {
        /* the common tile: the digit bins ARE the key counts */
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            atomicAdd(&bins[__builtin_amdgcn_ubfe(mine[j], idBits, digitBits)], 1u);
    }
    else
    {
        /* a lane's last tile, or one across low parts: the counts are gathered per (low part, top digit) for the first
         * KEY_COUNT_SLOTS low parts of the tile; keys of further ones (tiny groups) go straight to memory */
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            if (at + j * 64 < tileCount)
            {
                const uint32_t digit = __builtin_amdgcn_ubfe(mine[j], idBits, digitBits);
                atomicAdd(&bins[digit], 1u);
                if (!oneLow)
                {
                    const uint32_t low = lowPartAt(sLow, lowFirst, numLow, tileFirst + at + j * 64);
                    const uint32_t slot = low - lowFirst;
                    if (slot < KEY_COUNT_SLOTS)
                        atomicAdd(&keyBins[slot * CMD_BINS + digit], 1u);
                    else
                        atomicAdd(&A.keyCounts[(digit << shift) | low], 1u);
                }
            }
    }
    __syncthreads();
    const uint32_t d = threadIdx.x;
    if (d < numBins)
    {
        const uint32_t c = bins[d];
        A.hist[(uint64_t) d * A.numTiles + tile] = c;
        if (oneLow && c != 0)
            atomicAdd(&A.keyCounts[(d << shift) | lowFirst], c);
    }
    if (!oneLow)
#pragma unroll
        for (uint32_t k = threadIdx.x; k < KEY_COUNT_SLOTS * CMD_BINS; k += PRIM_BLOCK)
        {
            const uint32_t c = keyBins[k];
            if (c != 0)
                atomicAdd(&A.keyCounts[((k & (CMD_BINS - 1u)) << shift) | (lowFirst + (k >> ENT_BIN_BITS))], c);
        }
}

struct CommandScatterArgs
{
    const uint32_t *words;
    uint32_t *commands;
    const uint32_t *hist;
    const uint32_t *digitTotals;
    uint32_t n;
    const uint32_t *nDev;
    uint32_t numTiles;
    const uint32_t *keyBase;    /* the id of sorted rank r with key k goes to commands[1 + r + keyBase[k]] */
    const uint32_t *lowBase;
    uint32_t numKeys;           /* keyBase[0 .. numKeys) */
    uint32_t valueBias;         /* what goes out is id + valueBias */
};

/* The ranking and the tile in its new order live in the same 16 KB: the match words and runs are dead once every element
 * knows its place.  With the small tables 18 KB: eight workgroups to a CU, where the template's 30 KB allowed five. */
struct CommandTileLds
{
    union
    {
        struct
        {
            unsigned long long match[PRIM_WAVES][CMD_BINS];    /* per wave and digit: the lanes that hold the digit this round */
            uint32_t run[PRIM_WAVES][CMD_BINS];                 /* ... the wave's elements with the digit so far; then where its
                                                                 * first goes in the tile */
        } rank;
        uint32_t tile[SORT_TILE];
    };
    uint32_t tileBase[CMD_BINS];        /* what takes a place in the tile to a command position */
    uint32_t low[CMD_BINS];             /* group begins, for tiles across low parts */
    uint32_t waveTotals[PRIM_WAVES], waveTotalsAll[PRIM_WAVES];
};

/* The stable rank of each of the wave's elements among the wave's elements with the same digit, round by round: every lane
 * ORs its bit into the digit's match word and reads the word back (LDS operations of a wave execute in order); the lanes
 * below it in the word come before it, and the run so far before them.  The first lane of a peer group stores the run's new
 * end and the cleared match word.  The kernel is bound by the LDS, more than half of whose cycles are bank conflicts between
 * the digits of a round (profiles/NOTES_last_pass.md), so what counts is how many lanes touch how many banks: a lane ORs its
 * bit into its HALF of the match word, a 32-bit operation (63.1 -> 61.1 us per launch against the 64-bit one), and every lane
 * of the group storing the same two values, with no divergent part, lost to the one lane per digit (65.6 against 63.1).
 * COUNTING IS RANKING: the runs start from zero, so after the last round run[digit] is the wave's count of the digit, and
 * no separate counting phase runs before the scan over the bins.  left: elements of the wave's span that exist (!FULL). */
template<bool FULL>
__device__ __forceinline__ void commandRounds(CommandTileLds &s, const uint32_t (&word)[SORT_ITEMS], uint32_t (&rank)[SORT_ITEMS],
                                              uint32_t idBits, uint32_t digitBits, uint32_t left)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *const match = s.rank.match[wave];
    uint32_t *const run = s.rank.run[wave];
    const uint32_t half = lane >> 5, bit = 1u << (lane & 31u);
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; j++)
    {
        const uint32_t digit = __builtin_amdgcn_ubfe(word[j], idBits, digitBits);
        const bool valid = FULL || (uint32_t) j * 64 + lane < left;
        if (valid)
            atomicOr(reinterpret_cast<uint32_t *>(&match[digit]) + half, bit);
        __builtin_amdgcn_wave_barrier();
        rank[j] = 0;
        if (valid)
        {
            const unsigned long long peers = match[digit];
            const uint32_t before = run[digit];
            const uint32_t below = popcBelow(peers);
            rank[j] = before + below;
            if (below == 0)
            {
                run[digit] = before + (uint32_t) __popcll(peers);
                match[digit] = 0ull;
            }
        }
        /* LDS operations of one wave complete in program order, so the next round sees the update */
        __builtin_amdgcn_wave_barrier();
    }
}

/* ids out in tile-sorted order, each digit's run one contiguous burst; the tile lies in ONE low part, whose share of the
 * command position is in tileBase already */
template<bool FULL>
__device__ __forceinline__ void commandOut(const CommandTileLds &s, uint32_t *commands, uint32_t tileCount, uint32_t idBits,
                                           uint32_t digitBits, uint32_t valueBias)
{
    const uint32_t idMask = (1u << idBits) - 1u;
#pragma unroll
    for (int k = 0; k < SORT_ITEMS; k++)
    {
        const uint32_t p = threadIdx.x + k * PRIM_BLOCK;
        if (FULL || p < tileCount)
        {
            const uint32_t w = s.tile[p];
            commands[s.tileBase[__builtin_amdgcn_ubfe(w, idBits, digitBits)] + p] = (w & idMask) + valueBias;
        }
    }
}

__global__ __launch_bounds__(PRIM_BLOCK) void commandScatterKernel(Lanes<CommandScatterArgs> lanes, uint32_t shift,
                                                                   uint32_t digitBits, uint32_t idBits)
{
    __shared__ CommandTileLds s;
    const CommandScatterArgs A = lanes.a[blockIdx.y];
    if (blockIdx.x >= A.numTiles)
        return;
    uint32_t n = A.n;
    if (A.nDev != nullptr && *A.nDev < n)
        n = *A.nDev;
    const uint32_t tile = tileOfWorkgroup(blockIdx.x, A.numTiles);     /* its words of the [digit][tile] array: one L2's */
    const uint32_t tileFirst = tile * SORT_TILE;
    if (tileFirst >= n)
        return;
    const uint32_t tileCount = n - tileFirst < SORT_TILE ? n - tileFirst : (uint32_t) SORT_TILE;
    const bool full = tileCount == SORT_TILE;
    const uint32_t numBins = 1u << digitBits, numLow = 1u << shift;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t at = wave * SORT_WAVE_SPAN + lane;           /* the thread's first element in the tile */
    const uint32_t left = tileCount > wave * SORT_WAVE_SPAN ? tileCount - wave * SORT_WAVE_SPAN : 0u;
    /* Everything the workgroup reads that does not depend on another read is requested here, together: the group begins
     * (first: the one read that depends on another waits for them alone), its words, and the digit total and tile offset of
     * the bin this thread owns in the scan below. */
    uint32_t lowFirst, myBegin;
    bool oneLow;
    const uint32_t *const words = A.words + tileFirst + at;
    uint32_t word[SORT_ITEMS];
    const uint32_t d = threadIdx.x;
    const bool myBin = d < numBins;
    lowPartsOfTile(A.lowBase, numLow, tileFirst, tileFirst + tileCount - 1, lowFirst, oneLow, myBegin);
    if (full)
    {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            word[j] = words[j * 64];
    }
    else
    {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            word[j] = (uint32_t) j * 64 + lane < left ? words[j * 64] : 0u;
    }
    const uint32_t totalOf = myBin ? A.digitTotals[d] : 0u;
    const uint32_t histOf = myBin ? A.hist[(uint64_t) d * A.numTiles + tile] : 0u;
    /* a tile in one low part: a digit is a key, and 1 + keyBase[key] is folded into the digit's base -- 256 loads per tile
     * instead of one per element.  (Keys at or above numKeys are no node's: no element has them.) */
    const uint32_t myKey = (d << shift) | lowFirst;
    const uint32_t keyBaseOf = A.keyBase[myKey < A.numKeys ? myKey : 0u];
    const uint32_t fold = oneLow ? 1u + keyBaseOf : 0u;
    /* every wave clears its own rows: no barrier before the rounds */
#pragma unroll
    for (uint32_t k = lane; k < CMD_BINS; k += 64)
    {
        s.rank.match[wave][k] = 0ull;
        s.rank.run[wave][k] = 0u;
    }
    s.low[threadIdx.x] = myBegin;
    __builtin_amdgcn_wave_barrier();
    uint32_t rank[SORT_ITEMS];
    if (full)
        commandRounds<true>(s, word, rank, idBits, digitBits, left);
    else
        commandRounds<false>(s, word, rank, idBits, digitBits, left);
    __syncthreads();
    /* tile-local exclusive prefix over the digits (thread d owns bin d), and of every (wave, digit) */
    {
        uint32_t c[PRIM_WAVES], mine = 0;
#pragma unroll
        for (int w = 0; w < PRIM_WAVES; w++)
        {
            c[w] = s.rank.run[w][d];
            mine += c[w];
        }
        const uint32_t incl = waveInclusiveScan(mine), inclAll = waveInclusiveScan(totalOf);
        if (lane == 63)
        {
            s.waveTotals[wave] = incl;
            s.waveTotalsAll[wave] = inclAll;
        }
        __syncthreads();
        uint32_t run = incl - mine, base = inclAll - totalOf;
        for (uint32_t w = 0; w < wave; w++)
        {
            run += s.waveTotals[w];
            base += s.waveTotalsAll[w];
        }
        s.tileBase[d] = base + histOf - run + fold;
#pragma unroll
        for (int w = 0; w < PRIM_WAVES; w++)
        {
            s.rank.run[w][d] = run;
            run += c[w];
        }
    }
    __syncthreads();
    /* every element's place in the tile-sorted sequence: its (wave, digit)'s first + its rank among them */
    uint32_t dst[SORT_ITEMS];
#pragma unroll
    for (int j = 0; j < SORT_ITEMS; j++)
        dst[j] = s.rank.run[wave][__builtin_amdgcn_ubfe(word[j], idBits, digitBits)] + rank[j];
    __syncthreads();
    /* ... and the words go there, over the ranking's tables */
    if (full)
    {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            s.tile[dst[j]] = word[j];
    }
    else
    {
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            if ((uint32_t) j * 64 + lane < left)
                s.tile[dst[j]] = word[j];
    }
    __syncthreads();
    if (oneLow)         /* (uniform over the workgroup) */
    {
        if (full)
            commandOut<true>(s, A.commands, tileCount, idBits, digitBits, A.valueBias);
        else
            commandOut<false>(s, A.commands, tileCount, idBits, digitBits, A.valueBias);
        return;
    }
    /* A tile across low parts: what travels behind the words through the tile's reorder is the low part of every element's
     * key, and the command position takes one gather per element. */
    const uint32_t idMask = (1u << idBits) - 1u;
#pragma unroll
    for (int k = 0; k < SORT_ITEMS; k++)
    {
        const uint32_t p = threadIdx.x + k * PRIM_BLOCK;
        word[k] = p < tileCount ? s.tile[p] : 0u;
    }
    __syncthreads();
    {
        uint32_t low = lowFirst;
#pragma unroll
        for (int j = 0; j < SORT_ITEMS; j++)
            if ((uint32_t) j * 64 + lane < left)
            {
                low = lowPartAt(s.low, low, numLow, tileFirst + at + (uint32_t) j * 64);
                s.tile[dst[j]] = low;
            }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SORT_ITEMS; k++)
    {
        const uint32_t p = threadIdx.x + k * PRIM_BLOCK;
        if (p < tileCount)
        {
            const uint32_t digit = __builtin_amdgcn_ubfe(word[k], idBits, digitBits);
            const uint32_t key = (digit << shift) | s.tile[p];
            A.commands[s.tileBase[digit] + p + 1u + A.keyBase[key]] = (word[k] & idMask) + A.valueBias;
        }
    }
}

/* countCommands (kernels/octree.cl:230-239) as the scan's producer.  The reference leaves the
 * last indicator unwritten; an exclusive scan never reads it, so any value serves. */
struct IndicatorIn
{
    const uint32_t *keys;
    const uint32_t *n;          /* number of entries, on the device */
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        if (i + 1 >= *n)
            return 1u;
        return keys[i] != keys[i + 1] ? 3u : 1u;
    }
};

/* writeSplatIds (kernels/octree.cl:256-279) as the scan's consumer: cpos is the exclusive prefix. */
struct SplatIdsOut
{
    int32_t *commands, *start, *jumpPos;
    const uint32_t *keys, *ids;
    const uint32_t *n;
    __device__ __forceinline__ void operator()(uint64_t pos, uint32_t cpos, uint32_t) const
    {
        const uint32_t curKey = keys[pos];
        if (curKey != 0xFFFFFFFFu)
        {
            commands[cpos] = (int32_t) ids[pos];
            const uint32_t prevKey = pos > 0 ? keys[pos - 1] : 0xFFFFFFFFu;
            const uint32_t nextKey = pos + 1 < *n ? keys[pos + 1] : 0xFFFFFFFFu;
            if (prevKey != curKey)
                start[curKey] = (int32_t) (cpos - 1);
            if (curKey != nextKey)
                jumpPos[curKey] = (int32_t) (cpos + 1);
        }
    }
};

/*
 * writeStartTop + writeStart for all levels in one launch (kernels/octree.cl:292-341, loop
 * src/splat_tree_cl.cpp:320-331).  The reference walks levels coarse to fine and hands each node
 * its parent's start.  Unrolled, that value is: the start of the nearest NON-EMPTY strict ancestor,
 * or -1.  start[] of a non-empty node is written by writeSplatIds and never changes, so every node
 * can fetch it independently.
 */
/*
 * The command list without a pass over the entries (round 4).  In the sorted entry list a node's ids are one run, and
 * writeSplatIds (kernels/octree.cl:256-279) puts the id of sorted rank r at command position 1 + r + 2 * (non-empty nodes
 * before the id's node): the scan of countCommands' 1 / 3 indicators (src/splat_tree_cl.cpp:310-317) is that sum, entry by
 * entry.  With the number of entries of every node at hand -- the last pass's histogram kernel counts whole keys on the way
 * (commandHistKernel above; sortHistKernel<KEY_COUNTS> for entries of two words) -- a scan over the NODES (37 449 of them
 * for the default tree, not 7 million entries) gives each node its first rank and the number of non-empty nodes before it,
 * hence start[] and the jump slots of the non-empty nodes (NodeOut below), and the last scatter pass of the sort writes
 * every id straight to its command position (commandScatterKernel; sortScatterKernel<SPREAD> for two words): the sorted
 * (key, id) arrays are never written and countCommands / scan / writeSplatIds do not run.  `commands` and `start` are the
 * reference's, word for word (tests/test_gpu_tree.py, tests/test_gpu_last_pass.py).
 */
struct NodeIn
{
    const uint32_t *counts;
    __device__ __forceinline__ U3 operator()(uint64_t i) const
    {
        const uint32_t c = counts[i];
        return U3{c, c != 0 ? 1u : 0u, 0u};
    }
};

struct NodeOut
{
    int32_t *start, *jumpPos;
    uint32_t *nodeBase;
    __device__ __forceinline__ void operator()(uint64_t i, U3 excl, U3 val) const
    {
        if (val.a != 0)
        {
            /* first id at 1 + excl.a + 2 excl.b: start = that - 1 (octree.cl:272-274), the jump slot behind the last id (:275-277) */
            const uint32_t first = excl.a + 2 * excl.b;
            start[i] = (int32_t) first;
            jumpPos[i] = (int32_t) (first + val.a + 1);
            nodeBase[i] = 2 * excl.b;
        }
        else
            jumpPos[i] = -1;            /* fill(jumpPos, -1), kernels/octree.cl:346 */
    }
};

struct WriteStartArgs
{
    int32_t *start, *commands;
    const int32_t *jumpPos;
};

__global__ __launch_bounds__(256) void writeStartKernel(Lanes<WriteStartArgs> lanes, LevelOffsets levelOffsets, int minShift,
                                                        int maxShift, uint32_t numStart)
{
    const WriteStartArgs A = lanes.a[blockIdx.y];
    int32_t *const start = A.start, *const commands = A.commands;
    const int32_t *const jumpPos = A.jumpPos;
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= numStart)
        return;
    int level = minShift;
    while (level < maxShift && p >= levelOffsets.v[level + 1])
        level++;
    uint32_t code = p - levelOffsets.v[level];
    int32_t prev = -1;
    for (int l = level + 1; l <= maxShift; l++)
    {
        code >>= 3;
        const uint32_t a = levelOffsets.v[l] + code;
        if (jumpPos[a] >= 0)
        {
            prev = start[a];
            break;
        }
    }
    const int32_t jp = jumpPos[p];
    if (jp >= 0)
    {
        commands[jp] = prev;
        commands[start[p]] = jp;
    }
    else
        start[p] = prev;
}

/* fill(jumpPos, -1), kernels/octree.cl:346, for every lane */
__global__ __launch_bounds__(256) void fillKernel(Lanes<int32_t *> lanes, uint32_t n, int32_t value)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        lanes.a[blockIdx.y][i] = value;
}

__global__ void testHelpersKernel(int op, const int32_t *iargs, const float *fargs, uint32_t *out)
{
    if (op == 0)
        out[0] = makeCodeLoop(iargs[0], iargs[1], iargs[2]);
    else if (op == 1)
        out[0] = (uint32_t) levelShift(iargs[0], iargs[1], iargs[2], iargs[3], iargs[4], iargs[5]);
    else if (op == 2)
    {
        float r = pointBoxDist2(fargs[0], fargs[1], fargs[2], fargs[3], fargs[4], fargs[5], fargs[6], fargs[7], fargs[8]);
        out[0] = __float_as_uint(r);
    }
    else if (op == 3)
        out[0] = makeCode(iargs[0], iargs[1], iargs[2]);   /* fast path must agree with the loop form */
}

int runTestHelper(mlsgpu_ctx *ctx, int op, const int32_t *iargs, int ni, const float *fargs, int nf, uint32_t *out)
{
    DeviceArray<int32_t> dI;
    DeviceArray<float> dF;
    DeviceArray<uint32_t> dO;
    HIP_CHECK(hipSetDevice(ctx->device));
    PROPAGATE(dI.alloc(16));
    PROPAGATE(dF.alloc(16));
    PROPAGATE(dO.alloc(4));
    if (ni) HIP_CHECK(hipMemcpyAsync(dI, iargs, ni * 4, hipMemcpyHostToDevice, ctx->stream));
    if (nf) HIP_CHECK(hipMemcpyAsync(dF, fargs, nf * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(testHelpersKernel, dim3(1), dim3(1), 0, ctx->stream, op, (const int32_t *) dI, (const float *) dF, dO.get());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, dO, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MLSGPU_OK;
}

} // namespace

/* ------------------------------------------------------------------ C-ABI */

/* device memory only: the entry mailbox is pinned host memory */
MLSGPU_API uint64_t mlsgpu_hip_tree_resource_usage(uint64_t maxLevels, uint64_t maxSplats)
{
    uint64_t bytes = 0;
    mlsgpu_tree(maxLevels, maxSplats).buffers([&](auto &array, uint64_t n) {
        bytes += array.bytes(n);
        return MLSGPU_OK;
    });
    return bytes;
}

MLSGPU_API int mlsgpu_hip_tree_create(mlsgpu_ctx *ctx, uint64_t maxLevels, uint64_t maxSplats, mlsgpu_tree **out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(1 <= maxSplats && maxSplats <= MLSGPU_TREE_MAX_SPLATS, MLSGPU_ERR_LENGTH);   /* src/splat_tree_cl.cpp:106 */
    REQUIRE(1 <= maxLevels && maxLevels <= MLSGPU_TREE_MAX_LEVELS, MLSGPU_ERR_LENGTH);   /* :107 */
    HIP_CHECK(hipSetDevice(ctx->device));
    std::unique_ptr<mlsgpu_tree> t(new mlsgpu_tree(maxLevels, maxSplats));
    t->ctx = ctx;
    PROPAGATE(t->buffers([](auto &array, uint64_t n) { return array.alloc(n); }));
    PROPAGATE(t->entryBox.create());
    *out = t.release();
    return MLSGPU_OK;
}

MLSGPU_API void mlsgpu_hip_tree_destroy(mlsgpu_tree *t)
{
    if (!t)
        return;
    hipSetDevice(t->ctx->device);
    delete t;
}

/* SplatTreeCL::enqueueBuild (src/splat_tree_cl.cpp:269-335) for the buckets of a batch in lock-step: the trees (one per
 * lane, same levels, one context) are built by ONE set of launches whose workgroups pick their lane by blockIdx.y; the
 * entry counts of all lanes come back through one mailbox publication.  A single build is a batch of one. */
static int treeBuildBatch(mlsgpu_tree *const *trees, const mlsgpu_tree_build *reqs, uint32_t count, uint32_t subsamplingShift)
{
    REQUIRE(trees != nullptr && reqs != nullptr && count >= 1 && count <= MAX_LANES, MLSGPU_ERR_INVALID);
    mlsgpu_tree *const t0 = trees[0];
    REQUIRE(t0 != nullptr, MLSGPU_ERR_INVALID);
    mlsgpu_ctx *ctx = t0->ctx;
    /* src/splat_tree_cl.cpp:277-281 */
    REQUIRE(t0->maxLevels + subsamplingShift - 1 < 31, MLSGPU_ERR_LENGTH);
    const uint32_t maxSize = 1u << (t0->maxLevels + subsamplingShift - 1);
    for (uint32_t k = 0; k < count; k++)
    {
        const mlsgpu_tree *t = trees[k];
        const mlsgpu_tree_build &r = reqs[k];
        REQUIRE(t != nullptr && r.dSplats != nullptr, MLSGPU_ERR_INVALID);
        REQUIRE(t->ctx == ctx && t->maxLevels == t0->maxLevels, MLSGPU_ERR_INVALID);
        for (uint32_t j = 0; j < k; j++)
            REQUIRE(trees[j] != t, MLSGPU_ERR_INVALID);
        REQUIRE(r.numSplats <= t->maxSplats, MLSGPU_ERR_LENGTH);
        REQUIRE(r.firstSplat < 0xFFFFFFFFull - r.numSplats, MLSGPU_ERR_LENGTH);
        REQUIRE(r.size[0] <= maxSize && r.size[1] <= maxSize && r.size[2] <= maxSize, MLSGPU_ERR_LENGTH);
    }
    const int maxShift = (int) (t0->maxLevels + subsamplingShift - 1);
    const int minShift = (int) subsamplingShift < maxShift ? (int) subsamplingShift : maxShift;
    HIP_CHECK(hipSetDevice(ctx->device));

    LevelOffsets lo;
    std::memset(&lo, 0, sizeof(lo));
    uint64_t pos = 0;
    for (int i = minShift; i <= maxShift; i++)
    {
        lo.v[i] = (uint32_t) pos;
        pos += uint64_t(1) << (3 * (maxShift - i));
    }
    const uint32_t numStart = (uint32_t) pos;
    const uint32_t keyBits = (uint32_t) (3 * (maxShift - minShift) + 1);
    const uint32_t passes = sortPasses(keyBits, SortCaps<uint32_t>::MAX_DIGIT_BITS);
    const uint32_t perPass = (keyBits + passes - 1) / passes;
    static const bool fusedOff = getenv("MLSGPU_HIP_OCTREE_FUSED") != nullptr && atoi(getenv("MLSGPU_HIP_OCTREE_FUSED")) == 0;
    /* wider digits (deep trees) take the separate passes.  entryScatterKernel's ranking needs a digit of three bits or a
     * tree of one level (a one-bit key): every split sortPasses makes is one or the other, and one that were not would take
     * the separate passes too */
    const bool rankable = perPass >= ENT_MIN_DIGIT_BITS || maxShift == minShift;
    const bool fused = perPass <= ENT_BIN_BITS && keyBits <= ENT_KEY_BITS && rankable && !fusedOff;

    /* the command list straight from the sort's last pass (NodeIn / NodeOut above): for the fused front end with ONE pass left */
    const bool direct = fused && keyBits <= 2 * perPass;
    /* One word per entry between the two passes (entryScatterKernel / SortHistArgs): after the fused pass an entry's low
     * digit is its position, so the word holds the rest of the key above the splat's number inside the bucket -- when both
     * fit.  4 bytes less written and read again per entry (8 E of the 24 E the two passes move). */
    uint32_t idBits = 0;
    {
        const char *const env = getenv("MLSGPU_HIP_OCTREE_PACKED");      /* "0": two words per entry, as before (tests, A/B) */
        const bool packedOff = env != nullptr && atoi(env) == 0;
        uint64_t most = 1;
        for (uint32_t k = 0; k < count; k++)
            most = std::max<uint64_t>(most, reqs[k].numSplats);
        uint32_t bits = 1;
        while (bits < 32 && ((most - 1) >> bits) != 0)
            bits++;
        if (direct && !packedOff && (keyBits - perPass) + bits <= 32)
            idBits = bits;
    }
    /* packed words take the last pass's own kernels (commandHistKernel); "0": the sort's templates, as before (tests, A/B).
     * A top digit of zero bits (trees of one to three levels) is served by the same kernels: one bin. */
    bool lastPass = idBits != 0;
    if (const char *const env = getenv("MLSGPU_HIP_OCTREE_LAST_PASS"))
        lastPass = lastPass && atoi(env) != 0;
    for (uint32_t k = 0; k < count; k++)
    {
        mlsgpu_tree *t = trees[k];
        REQUIRE(numStart <= t->maxStart, MLSGPU_ERR_LENGTH);
        t->numLevels = (uint32_t) (maxShift - minShift + 1);
        t->dSplats = reqs[k].dSplats;
    }
    /* fill(jumpPos, -1), kernels/octree.cl:346 -- or, on the direct route, the node counters (NodeOut writes jumpPos) */
    const auto jump = packLanes<int32_t *>(count, [&](uint32_t k) {
        return direct ? reinterpret_cast<int32_t *>(trees[k]->dNodeCounts.get()) : trees[k]->dJumpPos.get();
    });
    LAUNCH(ctx, "kernel.octree.fill.time", fillKernel, dim3(divUp(numStart, 256), count), dim3(256), jump, numStart,
           (int32_t) (direct ? 0 : -1));

    /* the lanes that hold splats */
    uint32_t act[MAX_LANES], na = 0;
    for (uint32_t k = 0; k < count; k++)
        if (reqs[k].numSplats > 0)
            act[na++] = k;
    SortJob<uint32_t> sortJobs[MAX_LANES];
    uint64_t sortN[MAX_LANES];
    if (na > 0)
    {
        auto params = [&](uint32_t k) {
            const mlsgpu_tree_build &r = reqs[k];
            return EntryParams{r.dSplats, r.offset[0], r.offset[1], r.offset[2], lo, minShift, maxShift, (uint32_t) r.firstSplat,
                               trees[k]->mutate ? 1u : 0u};
        };
        if (fused)
        {
            /* writeEntries + the sort's first pass as one count / digit scan / scatter, see entryScatterKernel */
            const char *stat = "kernel.octree.writeEntries.time";
            auto tilesE = [&](uint32_t a) { return divUp(reqs[act[a]].numSplats, ENT_TILE); };
            auto digitTotals = [&](uint32_t a) { return trees[act[a]]->dHist + (uint64_t) (1u << perPass) * tilesE(a); };
            const auto eh = packLanes<EntryHistArgs>(na, [&](uint32_t a) {
                mlsgpu_tree *t = trees[act[a]];
                return EntryHistArgs{params(act[a]), t->dEntryNotes, t->dHist, tilesE(a), reqs[act[a]].numSplats};
            });
            const auto ds = packLanes<SortDigitScanArgs>(na, [&](uint32_t a) {
                return SortDigitScanArgs{trees[act[a]]->dHist, digitTotals(a), tilesE(a)};
            });
            const auto et = packLanes<EntryTotalArgs>(na, [&](uint32_t a) {
                return EntryTotalArgs{digitTotals(a), trees[act[a]]->dNumEntries, trees[act[a]]->dDigitBase};
            });
            const auto es = packLanes<EntryScatterArgs>(na, [&](uint32_t a) {
                mlsgpu_tree *t = trees[act[a]];
                return EntryScatterArgs{params(act[a]), t->dEntryNotes, t->dHist, digitTotals(a), tilesE(a), reqs[act[a]].numSplats,
                                        t->dKeysB, t->dValsB, idBits};
            });
            const uint32_t maxTiles = mostOfLanes(na, tilesE);
            LAUNCH(ctx, stat, entryHistKernel, dim3(maxTiles, na), dim3(ENT_THREADS), eh, perPass);
            LAUNCH(ctx, stat, (sortDigitScanKernel<uint32_t>), dim3(1u << perPass, na), dim3(PRIM_BLOCK), ds);
            /* The entry counts (2.4 .. 3.8 per splat on the BASELINE clouds, 8 at most) come back to the host: the remaining
             * sort pass and the command scan launch on n instead of 8N elements. */
            const uint32_t seq = t0->entryBox.reserve();
            LAUNCH(ctx, stat, entryTotalKernel, dim3(1), dim3(256), et, na, 1u << perPass, t0->entryBox.dev, seq);
            LAUNCH(ctx, stat, entryScatterKernel, dim3(maxTiles, na), dim3(ENT_THREADS), es, perPass);
            PROPAGATE(t0->entryBox.wait(ctx->stream));
            for (uint32_t a = 0; a < na; a++)
            {
                mlsgpu_tree *t = trees[act[a]];
                sortN[a] = t0->entryBox.payload()[a];
                sortJobs[a] = SortJob<uint32_t>{t->dKeysB, t->dValsB, t->dKeysA, t->dValsA, sortN[a], t->dHist, t->dNumEntries,
                                                SortResult<uint32_t>{nullptr, nullptr}};
            }
            if (!direct)
                PROPAGATE(radixSortBatch<uint32_t>(ctx, "kernel.octree.sort.time", sortJobs, na, keyBits, false, perPass));
        }
        else
        {
            /* writeEntries: count, scan, write compacted; the entry count stays on the device (t->dNumEntries) */
            typedef ScanJob<uint32_t, EntryCountIn, EntryMaskIn, EntryWriteOut> EntryJob;
            EntryJob jobs[MAX_LANES];
            const void *counts[MAX_LANES];
            for (uint32_t a = 0; a < na; a++)
            {
                const uint32_t k = act[a];
                mlsgpu_tree *t = trees[k];
                const EntryParams P = params(k);
                jobs[a] = EntryJob{EntryCountIn{P, t->dSlotMasks}, EntryMaskIn{t->dSlotMasks},
                                   EntryWriteOut{P, t->dSlotMasks, t->dKeysA, t->dValsA}, reqs[k].numSplats, 0u, t->dTileSums,
                                   t->dNumEntries, nullptr};
                counts[a] = t->dNumEntries;
            }
            PROPAGATE((exclusiveScanBatch<uint32_t, EntryCountIn, EntryMaskIn, EntryWriteOut>(
                ctx, "kernel.octree.writeEntries.time", jobs, na)));
            PROPAGATE(t0->entryBox.publishGather(ctx->stream, counts, na, 1));
            PROPAGATE(t0->entryBox.wait(ctx->stream));
            for (uint32_t a = 0; a < na; a++)
            {
                mlsgpu_tree *t = trees[act[a]];
                sortN[a] = t0->entryBox.payload()[a];
                sortJobs[a] = SortJob<uint32_t>{t->dKeysA, t->dValsA, t->dKeysB, t->dValsB, sortN[a], t->dHist, t->dNumEntries,
                                                SortResult<uint32_t>{nullptr, nullptr}};
            }
            PROPAGATE(radixSortBatch<uint32_t>(ctx, "kernel.octree.sort.time", sortJobs, na, keyBits, false));
        }
        if (direct)
        {
            /* the sort's last pass: histogram + whole-key counts */
            const uint32_t shift = perPass, digitBits = keyBits - perPass;
            const auto h = packLanes<SortHistArgs<uint32_t> >(na, [&](uint32_t a) {
                const SortJob<uint32_t> &j = sortJobs[a];
                return SortHistArgs<uint32_t>{j.keysA, j.dHist, j.n, j.nDev, sortTiles(j.n), trees[act[a]]->dNodeCounts,
                                              trees[act[a]]->dDigitBase, idBits};
            });
            const auto d = packLanes<SortDigitScanArgs>(na, [&](uint32_t a) {
                return SortDigitScanArgs{sortJobs[a].dHist, sortDigitTotals(sortJobs[a]), sortTiles(sortJobs[a].n)};
            });
            const auto ch = packLanes<CommandHistArgs>(na, [&](uint32_t a) {
                const SortJob<uint32_t> &j = sortJobs[a];
                return CommandHistArgs{j.keysA, j.dHist, (uint32_t) j.n, j.nDev, sortTiles(j.n), trees[act[a]]->dNodeCounts,
                                       trees[act[a]]->dDigitBase};
            });
            const uint32_t maxTiles = mostOfLanes(na, [&](uint32_t a) { return sortTiles(sortJobs[a].n); });
            if (maxTiles > 0)
            {
                if (lastPass)
                    LAUNCH(ctx, "kernel.octree.sort.time", commandHistKernel, dim3(maxTiles, na), dim3(PRIM_BLOCK), ch, shift, digitBits,
                           idBits);
                else
                    LAUNCH(ctx, "kernel.octree.sort.time", (sortHistKernel<uint32_t, true>), dim3(maxTiles, na), dim3(PRIM_BLOCK), h,
                           shift, digitBits);
                LAUNCH(ctx, "kernel.octree.sort.time", (sortDigitScanKernel<uint32_t>), dim3(1u << digitBits, na), dim3(PRIM_BLOCK), d);
            }
        }
        else
        {
            /* countCommands + scan(seed 1) + writeSplatIds, src/splat_tree_cl.cpp:310-317 */
            typedef ScanJob<uint32_t, IndicatorIn, IndicatorIn, SplatIdsOut> CommandJob;
            CommandJob cj[MAX_LANES];
            for (uint32_t a = 0; a < na; a++)
            {
                mlsgpu_tree *t = trees[act[a]];
                const SortResult<uint32_t> &sorted = sortJobs[a].result;
                const IndicatorIn in{sorted.keys, t->dNumEntries};
                cj[a] = CommandJob{in, in, SplatIdsOut{t->dCommands, t->dStart, t->dJumpPos, sorted.keys, sorted.vals, t->dNumEntries},
                                   sortN[a], 1u, t->dTileSums, (uint32_t *) nullptr, t->dNumEntries};
            }
            PROPAGATE((exclusiveScanBatch<uint32_t, IndicatorIn, IndicatorIn, SplatIdsOut>(ctx, "kernel.octree.scan.time", cj, na)));
        }
    }
    if (direct)
    {
        /* the scan over the NODES of every lane (a lane without splats has no entries anywhere: jumpPos = -1 throughout) */
        typedef ScanJob<U3, NodeIn, NodeIn, NodeOut> NodeJob;
        NodeJob nj[MAX_LANES];
        for (uint32_t k = 0; k < count; k++)
        {
            mlsgpu_tree *t = trees[k];
            const NodeIn in{t->dNodeCounts};
            nj[k] = NodeJob{in, in, NodeOut{t->dStart, t->dJumpPos, t->dNodeBase}, numStart, U3{0, 0, 0}, t->dNodeTiles, (U3 *) nullptr,
                            nullptr};
        }
        PROPAGATE((exclusiveScanBatch<U3, NodeIn, NodeIn, NodeOut>(ctx, "kernel.octree.scan.time", nj, count)));
        if (na > 0)
        {
            /* ... and the last scatter: every id to its command position */
            const uint32_t shift = perPass, digitBits = keyBits - perPass;
            const auto sc = packLanes<SortScatterArgs<uint32_t> >(na, [&](uint32_t a) {
                const SortJob<uint32_t> &j = sortJobs[a];
                mlsgpu_tree *t = trees[act[a]];
                return SortScatterArgs<uint32_t>{j.keysA, j.valsA, (uint32_t *) nullptr, reinterpret_cast<uint32_t *>(t->dCommands.get()), j.dHist,
                                                 sortDigitTotals(j), j.n, j.nDev, sortTiles(j.n), t->dNodeBase, t->dDigitBase, idBits,
                                                 (uint32_t) reqs[act[a]].firstSplat};
            });
            const auto cs = packLanes<CommandScatterArgs>(na, [&](uint32_t a) {
                const SortJob<uint32_t> &j = sortJobs[a];
                mlsgpu_tree *t = trees[act[a]];
                return CommandScatterArgs{j.keysA, reinterpret_cast<uint32_t *>(t->dCommands.get()), j.dHist, sortDigitTotals(j),
                                          (uint32_t) j.n, j.nDev, sortTiles(j.n), t->dNodeBase, t->dDigitBase, numStart,
                                          (uint32_t) reqs[act[a]].firstSplat};
            });
            const uint32_t maxTiles = mostOfLanes(na, [&](uint32_t a) { return sortTiles(sortJobs[a].n); });
            if (maxTiles > 0 && lastPass)
                LAUNCH(ctx, "kernel.octree.sort.time", commandScatterKernel, dim3(maxTiles, na), dim3(PRIM_BLOCK), cs, shift, digitBits,
                       idBits);
            else if (maxTiles > 0)
                LAUNCH(ctx, "kernel.octree.sort.time", (sortScatterKernel<uint32_t, false, 8, true>), dim3(maxTiles, na), dim3(PRIM_BLOCK), sc,
                       shift, digitBits);
        }
    }
    const auto ws = packLanes<WriteStartArgs>(count, [&](uint32_t k) {
        return WriteStartArgs{trees[k]->dStart, trees[k]->dCommands, trees[k]->dJumpPos};
    });
    LAUNCH(ctx, "kernel.octree.writeStart.time", writeStartKernel, dim3(divUp(numStart, 256), count), dim3(256),
           ws, lo, minShift, maxShift, numStart);
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_tree_build(mlsgpu_tree *t, mlsgpu_splat *dSplats, uint64_t firstSplat, uint64_t numSplats,
                                     const uint32_t size[3], const int32_t offset[3], uint32_t subsamplingShift)
{
    REQUIRE(t != nullptr && dSplats != nullptr && size != nullptr && offset != nullptr, MLSGPU_ERR_INVALID);
    mlsgpu_tree_build r;
    r.dSplats = dSplats;
    r.firstSplat = firstSplat;
    r.numSplats = numSplats;
    for (int i = 0; i < 3; i++)
    {
        r.size[i] = size[i];
        r.offset[i] = offset[i];
    }
    return treeBuildBatch(&t, &r, 1, subsamplingShift);
}

MLSGPU_API int mlsgpu_hip_tree_build_batch(mlsgpu_tree *const *trees, const mlsgpu_tree_build *builds, uint32_t count,
                                           uint32_t subsamplingShift)
{
    REQUIRE(trees != nullptr && builds != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(count >= 1 && count <= MLSGPU_MAX_BATCH, MLSGPU_ERR_LENGTH);
    return treeBuildBatch(trees, builds, count, subsamplingShift);
}

MLSGPU_API int mlsgpu_hip_tree_num_entries(mlsgpu_tree *t, uint64_t *out)
{
    REQUIRE(t != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    HIP_CHECK(hipSetDevice(t->ctx->device));
    uint32_t n = 0;
    HIP_CHECK(hipMemcpyAsync(&n, t->dNumEntries, 4, hipMemcpyDeviceToHost, t->ctx->stream));
    HIP_CHECK(hipStreamSynchronize(t->ctx->stream));
    *out = n;
    return MLSGPU_OK;
}

MLSGPU_API void mlsgpu_hip_tree_clear_splats(mlsgpu_tree *t) { if (t) t->dSplats = nullptr; }
MLSGPU_API const mlsgpu_splat *mlsgpu_hip_tree_splats(const mlsgpu_tree *t) { return t->dSplats; }
MLSGPU_API int mlsgpu_hip_tree_set_mutate(mlsgpu_tree *t, int mutate)
{
    REQUIRE(t != nullptr, MLSGPU_ERR_INVALID);
    t->mutate = mutate != 0;
    return MLSGPU_OK;
}
MLSGPU_API int mlsgpu_hip_tree_mutates(const mlsgpu_tree *t) { return t != nullptr && t->mutate ? 1 : 0; }
MLSGPU_API const int32_t *mlsgpu_hip_tree_commands(const mlsgpu_tree *t) { return t->dCommands; }
MLSGPU_API const int32_t *mlsgpu_hip_tree_start(const mlsgpu_tree *t) { return t->dStart; }
MLSGPU_API uint64_t mlsgpu_hip_tree_commands_size(const mlsgpu_tree *t) { return t->commandsSize; }
MLSGPU_API uint64_t mlsgpu_hip_tree_start_size(const mlsgpu_tree *t) { return t->maxStart; }
MLSGPU_API uint32_t mlsgpu_hip_tree_num_levels(const mlsgpu_tree *t) { return t->numLevels; }

MLSGPU_API int mlsgpu_hip_test_make_code(mlsgpu_ctx *ctx, int x, int y, int z, uint32_t *out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    int32_t a[3] = {x, y, z};
    uint32_t loopForm = 0, fast = 0;
    PROPAGATE(runTestHelper(ctx, 0, a, 3, nullptr, 0, &loopForm));
    if (x >= 0 && y >= 0 && z >= 0 && x < 1024 && y < 1024 && z < 1024)
    {
        PROPAGATE(runTestHelper(ctx, 3, a, 3, nullptr, 0, &fast));
        if (fast != loopForm)
            return setError(MLSGPU_ERR_INVALID, "makeCode fast path disagrees with loop form");
    }
    *out = loopForm;
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_test_level_shift(mlsgpu_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t *out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    int32_t a[6] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    uint32_t r = 0;
    PROPAGATE(runTestHelper(ctx, 1, a, 6, nullptr, 0, &r));
    *out = (int32_t) r;
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_test_point_box_dist2(mlsgpu_ctx *ctx, const float p[3], const float lo[3], const float hi[3],
                                               float *out)
{
    REQUIRE(ctx != nullptr && out != nullptr, MLSGPU_ERR_INVALID);
    float a[9] = {p[0], p[1], p[2], lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
    uint32_t r = 0;
    PROPAGATE(runTestHelper(ctx, 2, nullptr, 0, a, 9, &r));
    std::memcpy(out, &r, 4);
    return MLSGPU_OK;
}
