/*
 * Compact read-back of an indexed triangle mesh resident in HBM: the same mesh in fewer bytes for the link to the host, and the
 * host decoder that brings it back.  The reference has no counterpart.  The format (include/mlsgpu_hip.h, DESIGN.md "Compact
 * read-back") makes every byte of the blob a function of the input arrays and vertexBits: a minimum, a count, a scan or an OR
 * of disjoint bits, the same whatever the schedule.
 *
 *   extent     (vertexBits < 32) over the coordinates: those that are not finite, the integer minimum and maximum per axis
 *   plan       a wave per group of 64 triangles, a triangle per lane: the base by a wave minimum, the bit length of every
 *              value + 1 by a count of leading zeros, the exceptions of every width below the longest value's from ballots
 *              over those lengths, the arg-min cost; (base, width | exceptions << 8) per group, the width histogram and the
 *              exceptions added up
 *   scan       the record lengths, which follow from the plan, into the offset table          -- one read-back: the size --
 *   header     sixteen words
 *   vertices   (vertexBits < 32; a copy at 32) a wave per 64 vertices: 192 values of b bits are exactly 6 b words
 *   triangles  a wave per group: the rank of an exception in slot order from ballots, the 192 values of w bits into 6 w words
 *
 * The two packers share packTile: the wave clears its tile of LDS, every lane ORs its three values in (ds_or: the bits of two
 * values never overlap) and the tile leaves as whole words, lane after lane.
 *
 * What bounds the writes: the pack kernels write a record at the offset, and of the length, that the plan derived from the
 * same indices -- payload words from (n, w), exceptions from the same comparison v >= 2^w - 1 -- and the host compares the
 * scan's total with the capacity before anything is written.
 *
 * Scratch belongs to the call: 12 bytes per group (base, width and exceptions, offset), the scan's tile sums, 320 bytes of
 * counters.
 *
 * The decoder is plain host code.  It trusts nothing: one pass validates header, offsets and records (mlsgpu_hip.h lists
 * what), a second one writes.  Both are spread over std::threads by group and by vertex range.
 */
#include "primitives.hpp"

#include <cmath>
#include <thread>

using namespace mlsgpu;

namespace
{

enum
{
    GROUP = MLSGPU_COMPACT_GROUP,
    HEADER_WORDS = MLSGPU_COMPACT_HEADER_WORDS,
    WAVES = 4,                  /* groups per workgroup */
    TILE_WORDS = 3 * GROUP * 32 / 32,   /* 192 values of at most 32 bits */
    RECORD_MAX = 2 + TILE_WORDS,        /* w = 32; an exception costs a word, and w = 32 is taken before 192 of them are */
    EXTENT_BLOCK = 192,         /* a multiple of 3: a thread stays on its axis */
    LOOP_BLOCKS = 1024,
};
/* 32-bit words of the call: the extents as ordered integers, the length of all records */
enum { X_MIN = 0, X_MAX = 3, X_TOTAL = 6, X_WORDS = 8 };
/* 64-bit counts of the call */
enum { N_NON_FINITE = 0, N_EXCEPTIONS = 1, N_HIST = 2, N_WORDS = N_HIST + 33 };
typedef unsigned long long Count;

/* float bits <-> an unsigned integer of the same order (-0 below +0) */
__host__ __device__ inline uint32_t orderedOf(uint32_t bits) { return (bits >> 31) ? ~bits : bits | 0x80000000u; }
__host__ __device__ inline uint32_t bitsOf(uint32_t u) { return (u >> 31) ? u & 0x7FFFFFFFu : ~u; }
__host__ __device__ inline bool finiteBits(uint32_t bits) { return (bits & 0x7F800000u) != 0x7F800000u; }
/* the words of `values` values of `w` bits */
__host__ __device__ inline uint64_t streamWords(uint64_t values, uint32_t w) { return (values * w + 31) / 32; }

__global__ __launch_bounds__(EXTENT_BLOCK) void extentKernel(const uint32_t *bits, uint64_t n, uint32_t *ext, Count *counts)
{
    __shared__ uint32_t s[6], sBad;
    if (threadIdx.x < 3)
    {
        s[X_MIN + threadIdx.x] = 0xFFFFFFFFu;
        s[X_MAX + threadIdx.x] = 0u;
    }
    if (threadIdx.x == 0)
        sBad = 0;
    __syncthreads();
    uint32_t mn = 0xFFFFFFFFu, mx = 0u, bad = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * EXTENT_BLOCK + threadIdx.x; i < n; i += (uint64_t) gridDim.x * EXTENT_BLOCK)
    {
        const uint32_t b = bits[i];
        if (!finiteBits(b))
            bad++;
        else
        {
            const uint32_t u = orderedOf(b);
            mn = min(mn, u);
            mx = max(mx, u);
        }
    }
    const uint32_t axis = threadIdx.x % 3;      /* of every i above: block size and stride are multiples of 3 */
    atomicMin(&s[X_MIN + axis], mn);
    atomicMax(&s[X_MAX + axis], mx);
    if (bad)
        atomicAdd(&sBad, bad);
    __syncthreads();
    if (threadIdx.x < 3)
    {
        atomicMin(&ext[X_MIN + threadIdx.x], s[X_MIN + threadIdx.x]);
        atomicMax(&ext[X_MAX + threadIdx.x], s[X_MAX + threadIdx.x]);
    }
    if (threadIdx.x == 0 && sBad)
        atomicAdd(&counts[N_NON_FINITE], (Count) sBad);
}

__device__ __forceinline__ uint32_t waveMin(uint32_t v) { return ~waveMax(~v); }

/* the bit length of v + 1, 1..33: v is an exception at width w < 32 iff this exceeds w (v >= 2^w - 1 <=> v + 1 >= 2^w) */
__device__ __forceinline__ uint32_t lengthOf(uint32_t v) { return v == 0xFFFFFFFFu ? 33u : 32u - (uint32_t) __clz((int) (v + 1u)); }

/* the triangles of group g: how many, and this lane's (all ones where the lane has none: never the minimum before a live one) */
struct Corners
{
    uint32_t n, idx[3];
    bool live;
};
__device__ __forceinline__ Corners loadGroup(const uint32_t *tri, uint64_t T, uint64_t g, bool active, uint32_t lane)
{
    Corners c;
    const uint64_t first = g * GROUP;
    c.n = active ? (uint32_t) min((uint64_t) GROUP, T - first) : 0u;
    c.live = lane < c.n;
    for (int k = 0; k < 3; k++)
        c.idx[k] = c.live ? tri[3 * (first + lane) + k] : 0xFFFFFFFFu;
    return c;
}

__global__ __launch_bounds__(WAVES * 64) void planKernel(const uint32_t *tri, uint64_t T, uint32_t G, uint32_t *base, uint32_t *meta,
                                                         Count *counts)
{
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t groupsOfMyWidth = 0, exceptions = 0;       /* lane l counts the groups of width l */
    for (uint64_t g = (uint64_t) blockIdx.x * WAVES + wave; g < G; g += (uint64_t) gridDim.x * WAVES)     /* uniform in the wave */
    {
        const Corners c = loadGroup(tri, T, g, true, lane);
        const uint32_t b = waveMin(min(c.idx[0], min(c.idx[1], c.idx[2])));
        uint32_t len[3];
        for (int k = 0; k < 3; k++)
            len[k] = c.live ? lengthOf(c.idx[k] - b) : 0u;
        const uint32_t slots = 3 * c.n;
        /* from the longest value's width on nothing is an exception and a wider w only costs more: begin there */
        uint32_t bestW = min(waveMax(max(len[0], max(len[1], len[2]))), 32u), bestExc = 0;
        uint32_t bestCost = (uint32_t) streamWords(slots, bestW);       /* in words */
        for (uint32_t w = bestW - 1; w >= 1; w--)       /* downwards and <=: a tie goes to the smaller w */
        {
            const uint32_t exc = (uint32_t) (__popcll(__ballot(len[0] > w)) + __popcll(__ballot(len[1] > w)) + __popcll(__ballot(len[2] > w)));
            const uint32_t cost = (uint32_t) streamWords(slots, w) + exc;
            if (cost <= bestCost)
            {
                bestCost = cost;
                bestW = w;
                bestExc = exc;
            }
        }
        if (lane == 0)
        {
            base[g] = b;
            meta[g] = bestW | bestExc << 8;
        }
        groupsOfMyWidth += lane == bestW;
        exceptions += bestExc;
    }
    if (groupsOfMyWidth)        /* lanes 1..32 at most */
        atomicAdd(&counts[N_HIST + lane], (Count) groupsOfMyWidth);
    if (lane == 0 && exceptions)
        atomicAdd(&counts[N_EXCEPTIONS], (Count) exceptions);
}

/* the words of group g's record */
struct RecordLength
{
    const uint32_t *meta;
    uint64_t T;
    __device__ __forceinline__ uint32_t operator()(uint64_t g) const
    {
        const uint32_t n = (uint32_t) min((uint64_t) GROUP, T - g * GROUP), m = meta[g];
        return 2u + (uint32_t) streamWords(3 * n, m & 0xFFu) + (m >> 8);
    }
};

/* The wave's 3 n values of w bits, three per live lane in slot order, as `words` = ceil(3 n w / 32) words at dst.  Every thread
 * of the workgroup comes here (two barriers); a wave with nothing to write has words = 0 and no live lane. */
__device__ __forceinline__ void packTile(uint32_t *tile, const uint32_t val[3], bool live, uint32_t w, uint32_t words, uint32_t lane,
                                         uint32_t *dst)
{
    for (uint32_t j = lane; j < TILE_WORDS; j += 64)
        tile[j] = 0;
    __syncthreads();
    if (live)
        for (uint32_t k = 0; k < 3; k++)
        {
            const uint32_t bit = (3 * lane + k) * w, word = bit >> 5, sh = bit & 31;
            atomicOr(&tile[word], val[k] << sh);
            if (sh + w > 32)        /* then sh > 0, and the value's last bit is within the stream: word + 1 < words */
                atomicOr(&tile[word + 1], val[k] >> (32 - sh));
        }
    __syncthreads();
    for (uint32_t j = lane; j < words; j += 64)
        dst[j] = tile[j];
}

struct Quantiser
{
    double lo[3], scale[3], top;        /* scale = (2^b - 1) / d, 0 where d = 0; top = 2^b - 1 */
};

__global__ __launch_bounds__(WAVES * 64) void packVerticesKernel(const float *vertices, uint64_t V, uint32_t b, Quantiser Q, uint32_t *dst)
{
    __shared__ uint32_t tiles[WAVES][TILE_WORDS];
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t g = (uint64_t) blockIdx.x * WAVES + wave, first = g * GROUP;
    const uint32_t n = first < V ? (uint32_t) min((uint64_t) GROUP, V - first) : 0u;
    const bool live = lane < n;
    uint32_t q[3] = {0, 0, 0};
    if (live)
        for (int a = 0; a < 3; a++)
        {
            const double x = (double) vertices[3 * (first + lane) + a];
            double t = floor((x - Q.lo[a]) * Q.scale[a] + 0.5);
            t = t < 0.0 ? 0.0 : t;
            t = t > Q.top ? Q.top : t;
            q[a] = (uint32_t) t;
        }
    packTile(tiles[wave], q, live, b, (uint32_t) streamWords(3 * n, b), lane, dst + g * (3 * GROUP / 32) * b);
}

__global__ __launch_bounds__(WAVES * 64) void packTrianglesKernel(const uint32_t *tri, uint64_t T, uint32_t G, const uint32_t *base,
                                                                  const uint32_t *meta, const uint32_t *offsets, const uint32_t *total,
                                                                  uint32_t *offsetsOut, uint32_t *records)
{
    __shared__ uint32_t tiles[WAVES][TILE_WORDS];
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t g = (uint64_t) blockIdx.x * WAVES + wave;
    const bool active = g < G;
    const Corners c = loadGroup(tri, T, g, active, lane);
    const uint32_t b = active ? base[g] : 0u, m = active ? meta[g] : 1u, off = active ? offsets[g] : 0u;
    const uint32_t w = m & 0xFFu, escape = w < 32 ? (1u << w) - 1u : 0xFFFFFFFFu;
    uint32_t v[3], val[3];
    bool out[3];
    for (int k = 0; k < 3; k++)
    {
        v[k] = c.idx[k] - b;
        out[k] = c.live && w < 32 && v[k] >= escape;
        val[k] = out[k] ? escape : v[k];
    }
    /* exceptions in slot order: those of the lanes below, then this lane's own */
    uint32_t rank = popcBelow(__ballot(out[0])) + popcBelow(__ballot(out[1])) + popcBelow(__ballot(out[2]));
    const uint32_t words = (uint32_t) streamWords(3 * c.n, w);
    uint32_t *const rec = records + off;
    if (active && lane == 0)
    {
        rec[0] = b;
        rec[1] = m;
        offsetsOut[g] = off;
        if (g + 1 == G)
            offsetsOut[G] = *total;
    }
    packTile(tiles[wave], val, c.live, w, words, lane, rec + 2);
    for (int k = 0; k < 3; k++)
        if (out[k])
            rec[2 + words + rank++] = v[k];
}

struct Header
{
    uint32_t w[HEADER_WORDS];
};
/* the header, and the one offset of a mesh without triangles */
__global__ __launch_bounds__(64) void headerKernel(Header h, uint32_t *out, uint32_t *onlyOffset)
{
    if (threadIdx.x < HEADER_WORDS)
        out[threadIdx.x] = h.w[threadIdx.x];
    if (threadIdx.x == HEADER_WORDS && onlyOffset != nullptr)
        *onlyOffset = 0;
}

struct OffsetOut
{
    uint32_t *p;
    __device__ __forceinline__ void operator()(uint64_t g, uint32_t before, uint32_t) const { p[g] = before; }
};

float floatOf(uint32_t bits)
{
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}
uint32_t bitsOfFloat(float f)
{
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}
bool validBits(uint64_t b) { return b == 32 || (b >= 8 && b <= 24); }
/* d / (2^b - 1) per axis as the contract has it: 0 where d = 0 and at b = 32 */
void stepsOf(const float lo[3], const float hi[3], uint32_t b, double step[3], double scale[3])
{
    for (int a = 0; a < 3; a++)
    {
        const double d = (double) hi[a] - (double) lo[a], top = (double) ((uint64_t(1) << b) - 1);
        const bool flat = b == 32 || d == 0.0;
        step[a] = flat ? 0.0 : d / top;
        if (scale != nullptr)
            scale[a] = flat ? 0.0 : top / d;
    }
}

} // namespace

/* The encoder behind both entry points: the blob goes to dOut (device memory) or, through device scratch of its size, to
 * hostOut; whichever is given has `capacity` bytes. */
int mlsgpu::compactMesh(mlsgpu_ctx *ctx, const float *dVertices, uint64_t V, const uint32_t *dTriangles, uint64_t T, uint32_t b, void *dOut,
                        void *hostOut, uint64_t capacity, mlsgpu_compact_stats *stats)
{
    REQUIRE(ctx != nullptr && stats != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(validBits(b), MLSGPU_ERR_INVALID);
    REQUIRE(((uintptr_t) dOut & 3) == 0, MLSGPU_ERR_INVALID);
    const uint64_t G = (T + GROUP - 1) / GROUP;
    REQUIRE(V < (uint64_t(1) << 32) && T < ((uint64_t(1) << 32) + 2) / 3 && G * RECORD_MAX < (uint64_t(1) << 32), MLSGPU_ERR_LENGTH);
    REQUIRE(V == 0 || dVertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(T == 0 || dTriangles != nullptr, MLSGPU_ERR_INVALID);
    std::memset(stats, 0, sizeof(*stats));
    stats->numVertices = V;
    stats->numTriangles = T;
    stats->vertexBits = b;
    stats->groups = G;
    const uint64_t vertexWords = b == 32 ? 3 * V : streamWords(3 * V, b);
    stats->vertexBytes = 4 * vertexWords;

    HIP_CHECK(hipSetDevice(ctx->device));
    DeviceArray<uint32_t> ext, base, meta, offsets, tileSums, blob;
    DeviceArray<Count> counts;
    static const uint32_t initExt[X_WORDS] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0, 0};
    uint32_t hExt[X_WORDS];
    Count hCounts[N_WORDS];
    PROPAGATE(ext.alloc(X_WORDS));
    PROPAGATE(counts.alloc(N_WORDS));
    HIP_CHECK(hipMemcpyAsync(ext.get(), initExt, sizeof(initExt), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemsetAsync(counts.get(), 0, sizeof(hCounts), ctx->stream));
    if (b < 32 && V > 0)
        LAUNCH(ctx, "kernel.compact.extent", extentKernel, dim3(std::min(divUp(3 * V, EXTENT_BLOCK), (uint32_t) LOOP_BLOCKS)), dim3(EXTENT_BLOCK),
               reinterpret_cast<const uint32_t *>(dVertices), 3 * V, ext.get(), counts.get());
    if (G > 0)
    {
        PROPAGATE(base.alloc(G));
        PROPAGATE(meta.alloc(G));
        PROPAGATE(offsets.alloc(G));
        PROPAGATE(tileSums.alloc((uint64_t) scanTiles(G) + 1));
        if (ctx->timing)
            ctx->addValue("compact.scratch.bytes", (double) (3 * base.bytes(G) + tileSums.bytes((uint64_t) scanTiles(G) + 1) + sizeof(hExt) + sizeof(hCounts)));
        LAUNCH(ctx, "kernel.compact.plan", planKernel, dim3(std::min(divUp(G, WAVES), (uint32_t) LOOP_BLOCKS)), dim3(WAVES * 64), dTriangles, T,
               (uint32_t) G, base.get(), meta.get(), counts.get());
        PROPAGATE((exclusiveScan<uint32_t>(ctx, "kernel.compact.scan", RecordLength{meta.get(), T}, OffsetOut{offsets.get()}, G, 0u,
                                           tileSums.get(), ext.get() + X_TOTAL)));
    }
    HIP_CHECK(hipMemcpyAsync(hExt, ext.get(), sizeof(hExt), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(hCounts, counts.get(), sizeof(hCounts), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (hCounts[N_NON_FINITE] != 0)
        return setError(MLSGPU_ERR_INVALID, "mesh compact: %llu vertex coordinates are not finite", hCounts[N_NON_FINITE]);

    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    if (b < 32 && V > 0)
        for (int a = 0; a < 3; a++)
        {
            lo[a] = floatOf(bitsOf(hExt[X_MIN + a]));
            hi[a] = floatOf(bitsOf(hExt[X_MAX + a]));
        }
    Quantiser Q;
    stepsOf(lo, hi, b, stats->step, Q.scale);
    for (int a = 0; a < 3; a++)
        Q.lo[a] = (double) lo[a];
    Q.top = (double) ((uint64_t(1) << b) - 1);
    const uint64_t recordWords = hExt[X_TOTAL], totalWords = HEADER_WORDS + vertexWords + G + 1 + recordWords;
    stats->triangleBytes = 4 * (G + 1 + recordWords);
    stats->blobBytes = 4 * totalWords;
    stats->exceptions = hCounts[N_EXCEPTIONS];
    for (int w = 0; w < 33; w++)
        stats->widthHistogram[w] = hCounts[N_HIST + w];
    if ((dOut == nullptr && hostOut == nullptr) || capacity < stats->blobBytes)
        return setError(MLSGPU_ERR_LENGTH, "mesh compact: the output holds %llu bytes, the blob has %llu", (unsigned long long) capacity,
                        (unsigned long long) stats->blobBytes);

    if (dOut == nullptr)
    {
        PROPAGATE(blob.alloc(totalWords));
        dOut = blob.get();
    }
    uint32_t *const out = static_cast<uint32_t *>(dOut), *const offsetsOut = out + HEADER_WORDS + vertexWords;
    Header h;
    h.w[0] = MLSGPU_COMPACT_MAGIC;
    h.w[1] = MLSGPU_COMPACT_VERSION;
    h.w[2] = b;
    h.w[3] = GROUP;
    h.w[4] = (uint32_t) V;
    h.w[5] = (uint32_t) (V >> 32);
    h.w[6] = (uint32_t) T;
    h.w[7] = (uint32_t) (T >> 32);
    for (int a = 0; a < 3; a++)
    {
        h.w[8 + a] = bitsOfFloat(lo[a]);
        h.w[11 + a] = bitsOfFloat(hi[a]);
    }
    h.w[14] = (uint32_t) totalWords;
    h.w[15] = (uint32_t) (totalWords >> 32);
    LAUNCH(ctx, "kernel.compact.header", headerKernel, dim3(1), dim3(64), h, out, G == 0 ? offsetsOut : (uint32_t *) nullptr);
    if (V > 0 && b == 32)
        HIP_CHECK(hipMemcpyAsync(out + HEADER_WORDS, dVertices, 12 * V, hipMemcpyDeviceToDevice, ctx->stream));
    else if (V > 0)
        LAUNCH(ctx, "kernel.compact.vertices", packVerticesKernel, dim3(divUp(divUp(V, GROUP), WAVES)), dim3(WAVES * 64), dVertices, V, b, Q,
               out + HEADER_WORDS);
    if (G > 0)
        LAUNCH(ctx, "kernel.compact.triangles", packTrianglesKernel, dim3(divUp(G, WAVES)), dim3(WAVES * 64), dTriangles, T, (uint32_t) G,
               (const uint32_t *) base.get(), (const uint32_t *) meta.get(), (const uint32_t *) offsets.get(),
               (const uint32_t *) (ext.get() + X_TOTAL), offsetsOut, offsetsOut + G + 1);
    if (hostOut != nullptr)
        HIP_CHECK(hipMemcpyAsync(hostOut, out, stats->blobBytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));       /* the scratch goes with the call */
    return MLSGPU_OK;
}

MLSGPU_API int mlsgpu_hip_mesh_compact(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                       uint64_t numTriangles, uint32_t vertexBits, void *dOut, uint64_t capacityBytes,
                                       mlsgpu_compact_stats *stats)
{
    return compactMesh(ctx, dVertices, numVertices, dTriangles, numTriangles, vertexBits, dOut, nullptr, capacityBytes, stats);
}

/* ---------------------------------------------------------------- the host decoder: no HIP call below */

namespace
{

int badBlob(const char *what) { return setError(MLSGPU_ERR_FORMAT, "compact blob: %s", what); }

/* where the sections of a blob with a valid header lie */
struct Layout
{
    uint32_t b;
    uint64_t V, T, G, recordWords;
    const uint32_t *vertices, *offsets, *records;
    float lo[3], hi[3];
    double step[3];
};

/* The values of w <= 32 bits of a bit stream, one after the other from value `first`; a word is read when a value needs its
 * bits and not before, so the last read is the word of the last value's last bit. */
struct BitReader
{
    const uint32_t *next;
    uint64_t acc;
    uint32_t have, w;
    BitReader(const uint32_t *stream, uint64_t first, uint32_t w) : w(w)
    {
        const uint64_t bit = first * w;
        next = stream + (bit >> 5);
        acc = 0;
        have = 0;
        if (bit & 31)
        {
            acc = *next++ >> (bit & 31);
            have = 32 - (uint32_t) (bit & 31);
        }
    }
    inline uint32_t operator()()
    {
        if (have < w)
        {
            acc |= (uint64_t) *next++ << have;
            have += 32;
        }
        const uint32_t v = (uint32_t) (acc & ((uint64_t(1) << w) - 1));
        acc >>= w;
        have -= w;
        return v;
    }
};

int parseHeader(const void *blob, uint64_t bytes, Layout &L)
{
    REQUIRE(blob != nullptr && ((uintptr_t) blob & 3) == 0, MLSGPU_ERR_INVALID);
    if (bytes < 4 * HEADER_WORDS || bytes % 4 != 0)
        return badBlob("shorter than a header, or no whole number of words");
    const uint32_t *const w = static_cast<const uint32_t *>(blob);
    const uint64_t words = bytes / 4;
    if (w[0] != MLSGPU_COMPACT_MAGIC || w[1] != MLSGPU_COMPACT_VERSION || !validBits(w[2]) || w[3] != GROUP)
        return badBlob("magic, version, vertex bits or group size");
    L.b = w[2];
    L.V = w[4] | (uint64_t) w[5] << 32;
    L.T = w[6] | (uint64_t) w[7] << 32;
    if (L.V >= (uint64_t(1) << 32) || L.T >= ((uint64_t(1) << 32) + 2) / 3 || (w[14] | (uint64_t) w[15] << 32) != words)
        return badBlob("the sizes in the header");
    for (int a = 0; a < 3; a++)
    {
        const uint32_t lo = w[8 + a], hi = w[11 + a];
        if (L.b == 32 ? (lo | hi) != 0 : !finiteBits(lo) || !finiteBits(hi) || orderedOf(lo) > orderedOf(hi))
            return badBlob("the extents in the header");
        L.lo[a] = floatOf(lo);
        L.hi[a] = floatOf(hi);
    }
    stepsOf(L.lo, L.hi, L.b, L.step, nullptr);
    L.G = (L.T + GROUP - 1) / GROUP;
    const uint64_t vertexWords = L.b == 32 ? 3 * L.V : streamWords(3 * L.V, L.b), fixed = HEADER_WORDS + vertexWords + L.G + 1;
    if (fixed > words)
        return badBlob("the sections do not fit");
    L.recordWords = words - fixed;
    L.vertices = w + HEADER_WORDS;
    L.offsets = L.vertices + vertexWords;
    L.records = L.offsets + L.G + 1;
    if (L.offsets[0] != 0 || L.offsets[L.G] != L.recordWords)
        return badBlob("the first or last offset");
    return MLSGPU_OK;
}

/* One group: validated (WRITE = false: false if anything is wrong; *exceptions and hist updated) or written out.  Every read
 * is checked against the records' length before it happens. */
template<bool WRITE>
bool walkGroup(const Layout &L, uint64_t g, uint32_t *triangles, uint64_t *exceptions, uint64_t *hist)
{
    const uint64_t o0 = L.offsets[g], o1 = L.offsets[g + 1];
    const uint32_t n = (uint32_t) std::min<uint64_t>(GROUP, L.T - g * GROUP), slots = 3 * n;
    if (!WRITE && (o0 > o1 || o1 > L.recordWords || o1 - o0 < 2))
        return false;
    const uint32_t *const rec = L.records + o0;
    const uint32_t base = rec[0], w = rec[1] & 0xFFu, exc = rec[1] >> 8;
    if (!WRITE && (w < 1 || w > 32 || exc > slots || (w == 32 && exc != 0)))
        return false;
    const uint64_t words = streamWords(slots, w);
    if (!WRITE && o1 - o0 != 2 + words + exc)
        return false;
    const uint32_t *const tail = rec + 2 + words, escape = w < 32 ? (1u << w) - 1u : 0u;
    BitReader slot(rec + 2, 0, w);
    if (WRITE)
    {
        uint32_t *const out = triangles + 3 * GROUP * g;
        if (w == 32)
            for (uint32_t s = 0; s < slots; s++)
                out[s] = base + slot();
        else
            for (uint32_t s = 0, met = 0; s < slots; s++)
            {
                const uint32_t v = slot();
                out[s] = base + (v == escape ? tail[met++] : v);
            }
        return true;
    }
    /* the escapes number the exceptions, and neither the largest inline value nor an exception wraps */
    uint32_t met = 0, most = 0;
    for (uint32_t s = 0; s < slots; s++)
    {
        const uint32_t v = slot();
        const bool esc = w < 32 && v == escape;
        met += esc;
        most = std::max(most, esc ? 0u : v);
    }
    if (met != exc)
        return false;
    for (uint32_t j = 0; j < exc; j++)
        most = std::max(most, tail[j]);
    if ((uint64_t) base + most > 0xFFFFFFFFull)
        return false;
    *exceptions += exc;
    hist[w]++;
    return true;
}

void decodeVertices(const Layout &L, uint64_t v0, uint64_t v1, float *vertices)
{
    if (L.b == 32)
    {
        if (v1 > v0)
            std::memcpy(vertices + 3 * v0, L.vertices + 3 * v0, 12 * (v1 - v0));
        return;
    }
    const double lo[3] = {(double) L.lo[0], (double) L.lo[1], (double) L.lo[2]};
    BitReader q(L.vertices, 3 * v0, L.b);
    for (uint64_t v = v0; v < v1; v++)
        for (int a = 0; a < 3; a++)
            vertices[3 * v + a] = (float) (lo[a] + (double) q() * L.step[a]);
}

/* fn(part, first, last) over `parts` even ranges of [0, n), each on a thread of its own; the caller's runs the first */
template<typename Fn>
void spread(uint64_t n, uint32_t parts, Fn fn)
{
    std::vector<std::thread> pool;
    auto range = [&](uint32_t p) { return n / parts * p + std::min<uint64_t>(p, n % parts); };
    for (uint32_t p = 1; p < parts; p++)
    {
        try
        {
            pool.emplace_back(fn, p, range(p), range(p + 1));
        }
        catch (const std::system_error &)       /* no more threads to be had: here, then */
        {
            fn(p, range(p), range(p + 1));
        }
    }
    fn(0, range(0), range(1));
    for (std::thread &t : pool)
        t.join();
}

struct PartReport
{
    uint64_t exceptions = 0, hist[33] = {};
    bool ok = true;
};

/* header, offsets and every record, over `parts` threads; *stats (may be NULL) from what they counted */
int validate(const void *blob, uint64_t bytes, uint32_t parts, Layout &L, mlsgpu_compact_stats *stats)
{
    PROPAGATE(parseHeader(blob, bytes, L));
    std::vector<PartReport> reports(parts);
    spread(L.G, parts, [&](uint32_t p, uint64_t g0, uint64_t g1) {
        PartReport &r = reports[p];
        for (uint64_t g = g0; g < g1 && r.ok; g++)
            r.ok = walkGroup<false>(L, g, nullptr, &r.exceptions, r.hist);
    });
    for (const PartReport &r : reports)
        if (!r.ok)
            return badBlob("an offset or a group record");
    if (stats == nullptr)
        return MLSGPU_OK;
    std::memset(stats, 0, sizeof(*stats));
    stats->numVertices = L.V;
    stats->numTriangles = L.T;
    stats->vertexBits = L.b;
    stats->blobBytes = bytes;
    stats->vertexBytes = 4 * (uint64_t) (L.offsets - L.vertices);
    stats->triangleBytes = 4 * (L.G + 1 + L.recordWords);
    stats->groups = L.G;
    for (const PartReport &r : reports)
    {
        stats->exceptions += r.exceptions;
        for (int w = 0; w < 33; w++)
            stats->widthHistogram[w] += r.hist[w];
    }
    for (int a = 0; a < 3; a++)
        stats->step[a] = L.step[a];
    return MLSGPU_OK;
}

} // namespace

MLSGPU_API int mlsgpu_hip_compact_info(const void *blob, uint64_t bytes, mlsgpu_compact_stats *stats)
{
    REQUIRE(stats != nullptr, MLSGPU_ERR_INVALID);
    Layout L;
    return validate(blob, bytes, 1, L, stats);
}

MLSGPU_API int mlsgpu_hip_compact_decode(const void *blob, uint64_t bytes, float *vertices, uint32_t *triangles, uint32_t threads)
{
    const uint32_t parts = threads == 0 ? 8u : std::min(threads, 64u);
    Layout L;
    PROPAGATE(validate(blob, bytes, parts, L, nullptr));
    REQUIRE(L.V == 0 || vertices != nullptr, MLSGPU_ERR_INVALID);
    REQUIRE(L.T == 0 || triangles != nullptr, MLSGPU_ERR_INVALID);
    spread(L.G, parts, [&](uint32_t, uint64_t g0, uint64_t g1) {
        for (uint64_t g = g0; g < g1; g++)
            walkGroup<true>(L, g, triangles, nullptr, nullptr);
    });
    spread(L.V, parts, [&](uint32_t, uint64_t v0, uint64_t v1) { decodeVertices(L, v0, v1, vertices); });
    return MLSGPU_OK;
}
