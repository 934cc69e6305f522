/*
 * mlsgpu_hip.h -- C-ABI of the MI355X (gfx950) per-bucket device pipeline.
 *
 * The reference (bmerry/mlsgpu) has no C plugin interface for this path: its
 * boundary is the C++ class surface consumed by
 * DeviceWorkerGroupBase::Worker::operator() (src/workers.cpp:232-286), typed on
 * cl::Context / cl::CommandQueue / cl::Buffer / cl::Image2D.  This header is
 * the C-ABI a maintainer binds instead; each entry point cites the reference
 * interface it replaces.  mlsgpu_amd/host/ holds header-only C++ classes with
 * the reference's own names (SplatTreeCL, MlsFunctor, Marching, ...) built on
 * this ABI; INTEGRATION.md shows the reference-side changes.
 *
 * Conventions
 *  - every function returns MLSGPU_OK (0) or an error code; the text of the
 *    last error of the calling thread is mlsgpu_hip_last_error();
 *  - error classes follow the reference's exceptions: MLSGPU_ERR_LENGTH ~
 *    std::length_error, MLSGPU_ERR_INVALID ~ std::invalid_argument,
 *    MLSGPU_ERR_HIP ~ cl::Error, MLSGPU_ERR_NOMEM ~ CL_MEM_OBJECT_ALLOCATION_FAILURE;
 *  - objects are NOT thread-safe; one worker thread owns one context (= one
 *    HIP stream) and the objects made from it (src/mls.h:74-77,
 *    src/workers.h:183-206);
 *  - "d" prefixed pointers are device pointers on the context's device.
 */
#ifndef MLSGPU_HIP_H
#define MLSGPU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLSGPU_OK 0
#define MLSGPU_ERR_INVALID 1
#define MLSGPU_ERR_LENGTH 2
#define MLSGPU_ERR_HIP 3
#define MLSGPU_ERR_NOMEM 4
#define MLSGPU_ERR_CALLBACK 5
#define MLSGPU_ERR_DENSITY 6   /* Bucket::DensityError, src/bucket.h:52-65 */
#define MLSGPU_ERR_FORMAT 7    /* FastPly::FormatError, src/fast_ply.h:60-75 */

/* struct Splat, src/splat.h:40-46 == kernels/octree.cl:32-36 (32 bytes, AoS).
 * After mlsgpu_hip_tree_build the radius slot holds 1/radius^2 (octree.cl:193). */
typedef struct mlsgpu_splat
{
    float position[3];
    float radius;
    float normal[3];
    float quality;
} mlsgpu_splat;

/* MlsShape, src/mls.h:47-51 */
#define MLSGPU_SHAPE_SPHERE 0
#define MLSGPU_SHAPE_PLANE 1

/* Marching::Swathe (+ImageParams), src/marching.h:173-198.  The distance
 * field lives in a linear float buffer that is addressed exactly like the
 * reference's 2-D image: corner (x, y, z) is field[(y + z*zStride + zBias) * pitch + x]. */
typedef struct mlsgpu_swathe
{
    uint32_t width, height;
    uint32_t zStride;
    int32_t zBias;
    uint32_t zFirst, zLast;   /* closed interval of corner slices */
} mlsgpu_swathe;

/* DeviceKeyMesh, src/mesh.h:101-123: packed float xyz vertices, uint32 index
 * triplets, uint64 keys for all vertices (meaningful for external ones only);
 * internal vertices first. */
typedef struct mlsgpu_mesh
{
    float *dVertices;
    uint32_t *dTriangles;
    uint64_t *dVertexKeys;
    uint64_t numVertices;
    uint64_t numTriangles;
    uint64_t numInternalVertices;
} mlsgpu_mesh;

typedef struct mlsgpu_ctx mlsgpu_ctx;
typedef struct mlsgpu_tree mlsgpu_tree;
typedef struct mlsgpu_mls mlsgpu_mls;
typedef struct mlsgpu_marching mlsgpu_marching;
typedef struct mlsgpu_worker mlsgpu_worker;

/* Marching::Generator, src/marching.h:204-253.  enqueue() must enqueue (on
 * `stream`, a hipStream_t) work that fills slices zFirst..zLast of dField. */
typedef struct mlsgpu_generator
{
    uint32_t alignment[3];
    int (*enqueue)(void *user, void *stream, float *dField, uint64_t pitch, const mlsgpu_swathe *swathe);
    void *user;
} mlsgpu_generator;

/* Marching::OutputFunctor, src/marching.h:516-546.  The mesh is valid until
 * the functor returns (it may enqueue reads on `stream` and must synchronise
 * them itself, or copy with mlsgpu_hip_mesh_read). */
typedef int (*mlsgpu_output_fn)(void *user, void *stream, const mlsgpu_mesh *mesh);

const char *mlsgpu_hip_last_error(void);

/* ---- context: one device + one in-order stream (cl::Context + cl::CommandQueue of a worker,
 *      src/workers.cpp:207-221).  stream == NULL creates a private stream; otherwise the given
 *      hipStream_t (e.g. a torch stream) is used and not destroyed. ---- */
int mlsgpu_hip_ctx_create(int device, void *stream, mlsgpu_ctx **out);
void mlsgpu_hip_ctx_destroy(mlsgpu_ctx *ctx);
void *mlsgpu_hip_ctx_stream(mlsgpu_ctx *ctx);
int mlsgpu_hip_ctx_synchronize(mlsgpu_ctx *ctx);
/* Calls that work on the context keep their device scratch from call to call (mlsgpu_hip_bucket: the member lists, the kept
 * ranges and the counters of every recursion depth -- 24 GB behind a 10^9-splat cloud; the reference's Bucket::bucket
 * holds its counters and ranges on the host only for the duration of a call, src/bucket_impl.h:439-560).  This waits for the
 * context's stream and hands that memory back; lists handed to a callback must have been consumed.  Returns the error code. */
int mlsgpu_hip_ctx_release_scratch(mlsgpu_ctx *ctx);
int mlsgpu_hip_device_count(int *count);

/* Device / pinned memory helpers (CLH::PinnedMemory, src/clh.h:334-477; cl::Buffer). */
int mlsgpu_hip_malloc(mlsgpu_ctx *ctx, size_t bytes, void **dptr);
int mlsgpu_hip_free(mlsgpu_ctx *ctx, void *dptr);
int mlsgpu_hip_host_alloc(size_t bytes, void **hptr);
int mlsgpu_hip_host_free(void *hptr);
int mlsgpu_hip_memcpy_h2d(mlsgpu_ctx *ctx, void *dst, const void *src, size_t bytes, int async);
int mlsgpu_hip_memcpy_d2h(mlsgpu_ctx *ctx, void *dst, const void *src, size_t bytes, int async);
int mlsgpu_hip_memcpy_d2d(mlsgpu_ctx *ctx, void *dst, const void *src, size_t bytes);   /* async on the stream */
int mlsgpu_hip_memset(mlsgpu_ctx *ctx, void *dst, int value, size_t bytes);

/* Per-kernel device timing, the `--statistics-cl` facility (src/statistics_cl.cpp:62-160) with the
 * reference's stat names (kernel.octree.*.time, kernel.mls.processCorners.time, kernel.marching.*.time,
 * kernel.scaleBias.time).  Timing uses hipEvent pairs on the context's stream. */
int mlsgpu_hip_ctx_set_timing(mlsgpu_ctx *ctx, int enabled);
/* Synchronises, then returns total milliseconds and launch count of `name` since the last reset. */
int mlsgpu_hip_ctx_get_stat(mlsgpu_ctx *ctx, const char *name, double *totalMs, uint64_t *launches);
int mlsgpu_hip_ctx_reset_stats(mlsgpu_ctx *ctx);
/* Writes "name total_ms launches\n" lines; returns number of bytes needed.  The registry also carries the reference's
 * non-timer statistics of Marching under their own names (src/marching.cpp:350-352, always on): marching.overflow,
 * marching.slices.nonempty, marching.shipouts -- the SUM of the samples in the total_ms column, their number in the launches
 * column (Statistics::Variable's sum and n). */
size_t mlsgpu_hip_ctx_dump_stats(mlsgpu_ctx *ctx, char *buf, size_t bufSize);

/* ---- SplatTreeCL (src/splat_tree_cl.h:216-296) ---- */
#define MLSGPU_TREE_MAX_LEVELS 10                          /* src/splat_tree_cl.h:76 */
#define MLSGPU_TREE_MAX_SPLATS (((uint64_t) 1 << 31) / 16) /* src/splat_tree_cl.h:88 */
int mlsgpu_hip_tree_create(mlsgpu_ctx *ctx, uint64_t maxLevels, uint64_t maxSplats, mlsgpu_tree **out);
void mlsgpu_hip_tree_destroy(mlsgpu_tree *tree);
/* SplatTreeCL::resourceUsage: device bytes a tree of this capacity allocates. */
uint64_t mlsgpu_hip_tree_resource_usage(uint64_t maxLevels, uint64_t maxSplats);
/* SplatTreeCL::enqueueBuild, src/splat_tree_cl.cpp:269-335.  Enqueues on the context's stream, with one stream
 * synchronisation inside (the entry count sizes the sort); the tree is complete in stream order on return.  Borrows
 * dSplats until mlsgpu_hip_tree_clear_splats and MUTATES it (radius -> 1/radius^2). */
int mlsgpu_hip_tree_build(mlsgpu_tree *tree, mlsgpu_splat *dSplats, uint64_t firstSplat, uint64_t numSplats,
                          const uint32_t size[3], const int32_t offset[3], uint32_t subsamplingShift);
/* Batches: a device worker may take several buckets -- the SubItems of one WorkItem (src/workers.h:148-181), which the
 * reference's worker walks one by one (src/workers.cpp:232-286) -- through the path in lock-step.  Every kernel of the path
 * has a bucket dimension (blockIdx.y = bucket, per-bucket arguments in the kernel-argument segment), so a batch is ONE set
 * of launches and three host decisions; per bucket the results are those of the one-bucket entry points, bit for bit. */
#define MLSGPU_MAX_BATCH 8
typedef struct mlsgpu_tree_build
{
    mlsgpu_splat *dSplats;
    uint64_t firstSplat, numSplats;
    uint32_t size[3];
    int32_t offset[3];
} mlsgpu_tree_build;
/* SplatTreeCL::enqueueBuild for `count` buckets at once: trees[k] (distinct trees of one context and one depth) is built
 * from builds[k], arguments as mlsgpu_hip_tree_build.  One read-back of all the entry counts. */
int mlsgpu_hip_tree_build_batch(mlsgpu_tree *const *trees, const mlsgpu_tree_build *builds, uint32_t count,
                                uint32_t subsamplingShift);
/* mutate = 0: builds leave dSplats as they are (no radius -> 1/radius^2, kernels/octree.cl:193); mlsgpu_hip_mls_set then
 * makes processCorners take the reciprocal itself while it stages a splat -- the same expression on the same value, so the
 * field is bit-identical.  For callers whose splats stay resident over several builds.  Default 1: the reference's
 * behaviour. */
int mlsgpu_hip_tree_set_mutate(mlsgpu_tree *tree, int mutate);
int mlsgpu_hip_tree_mutates(const mlsgpu_tree *tree);
void mlsgpu_hip_tree_clear_splats(mlsgpu_tree *tree);
/* Measurement aid: (splat, node) entries of the last build (synchronises the stream). */
int mlsgpu_hip_tree_num_entries(mlsgpu_tree *tree, uint64_t *out);
const mlsgpu_splat *mlsgpu_hip_tree_splats(const mlsgpu_tree *tree);   /* getSplats   */
const int32_t *mlsgpu_hip_tree_commands(const mlsgpu_tree *tree);      /* getCommands */
const int32_t *mlsgpu_hip_tree_start(const mlsgpu_tree *tree);         /* getStart    */
uint64_t mlsgpu_hip_tree_commands_size(const mlsgpu_tree *tree);       /* elements allocated */
uint64_t mlsgpu_hip_tree_start_size(const mlsgpu_tree *tree);
uint32_t mlsgpu_hip_tree_num_levels(const mlsgpu_tree *tree);          /* getNumLevels */

/* ---- MlsFunctor (src/mls.h:79-170) ----
 * The functor owns one device allocation, which no resource_usage figure counts (the reference's functor has none): the table
 * of block descriptors its default kernel reads, 64 bytes per 8x8x8 block of the largest launch so far (of all its buckets,
 * for the first functor of mlsgpu_hip_mls_enqueue_batch): 2 MB for a 256^3 bucket.  It is allocated by the first enqueue, only
 * grows, and goes with mlsgpu_hip_mls_destroy. */
int mlsgpu_hip_mls_create(mlsgpu_ctx *ctx, int shape, mlsgpu_mls **out);
void mlsgpu_hip_mls_destroy(mlsgpu_mls *mls);
/* MlsFunctor::set(offset, tree, subsamplingShift), src/mls.cpp:91-94 */
int mlsgpu_hip_mls_set(mlsgpu_mls *mls, const int32_t offset[3], const mlsgpu_tree *tree, uint32_t subsamplingShift);
/* the private MlsFunctor::set(offset, splats, commands, start, shift) used by test/test_mls.cpp:475 */
int mlsgpu_hip_mls_set_buffers(mlsgpu_mls *mls, const int32_t offset[3], const mlsgpu_splat *dSplats,
                               const int32_t *dCommands, const int32_t *dStart, uint32_t subsamplingShift);
int mlsgpu_hip_mls_set_boundary_limit(mlsgpu_mls *mls, float limit);   /* src/mls.cpp:137-144 */
/* With explicit buffers (mlsgpu_hip_mls_set_buffers): 1 if the splats' radius slot still holds the radius, 0 (default) if
 * it holds 1/radius^2 as after a mutating build.  mlsgpu_hip_mls_set takes it from the tree. */
int mlsgpu_hip_mls_set_raw_radius(mlsgpu_mls *mls, int rawRadius);
/* MlsFunctor::enqueue, src/mls.cpp:101-135.  fieldRows = rows allocated in dField (bounds check). */
int mlsgpu_hip_mls_enqueue(mlsgpu_mls *mls, float *dField, uint64_t pitch, uint64_t fieldRows,
                           const mlsgpu_swathe *swathe);
/* Fills *gen so the functor can be passed to mlsgpu_hip_marching_generate (alignment = wgs = {8,8,8}). */
int mlsgpu_hip_mls_generator(mlsgpu_mls *mls, mlsgpu_generator *gen);
/* Selects the kernel: 5 = the default (sub-block culling + a bf16 matrix-core prefilter of the distance test; the
 * accumulation runs under the reference's own test), 4 = round 5's default (sub-block culling + one splat stream per
 * 2x2x2 cube of corners), 1 = the reference's structure (every corner walks every listed splat); 4 and 1 are kept for
 * A/B.  Bit-identical results.  Other values are MLSGPU_ERR_INVALID (0, 2 and 3 were intermediate designs of earlier
 * rounds). */
int mlsgpu_hip_mls_set_variant(mlsgpu_mls *mls, int variant);
/* Measurement aid: with a non-NULL device array of MLSGPU_MLS_STATS_WORDS uint64 the next enqueues run an instrumented
 * kernel that adds [0] listed splats (Sigma L of SURVEY 8d), [1] (corner, splat) distance tests executed, [2] hits (H);
 * and, for the default kernel, how its accumulation ("drain") loops use the 64 lanes of a wave -- a drain call runs as many
 * iterations as the LONGEST of its 64 lanes' hit lists: [3] drain calls, [4] iterations they ran (sum of the longest
 * list), [5] the iterations if every two consecutive calls of a wave were one call, [6] if a whole round of staged splats
 * were one call, [7] if a whole block were; [8 + n], n = 0 .. 32: lanes that had n hits in a drain call.  Lane
 * utilisation of the drain = [2] / (64 x [4]).  Kernel 5: [1] = (corner, splat) pairs the matrix prefilter evaluated,
 * [5] = 0, n = CANDIDATES of a lane in a drain call, [41] candidates the prefilter handed to the drain, [42] hits of the
 * reference's test that the prefilter missed (its superset property: must be 0).  Results are unchanged; NULL switches
 * back to the production kernel. */
#define MLSGPU_MLS_STATS_WORDS 43
int mlsgpu_hip_mls_set_stats(mlsgpu_mls *mls, uint64_t *dCounters);

/* ---- Marching (src/marching.h:494-608) ---- */
#define MLSGPU_MARCHING_MAX_DIMENSION 8192      /* src/marching.h:136 */
#define MLSGPU_MARCHING_MAX_CELL_BYTES 872      /* src/marching.h:96-100 */
int mlsgpu_hip_marching_create(mlsgpu_ctx *ctx, uint32_t maxWidth, uint32_t maxHeight, uint32_t maxDepth,
                               uint32_t maxSwathe, uint64_t meshMemory, const uint32_t alignment[3],
                               mlsgpu_marching **out);
void mlsgpu_hip_marching_destroy(mlsgpu_marching *m);
/* Marching::resourceUsage: device bytes a Marching of this capacity allocates. */
uint64_t mlsgpu_hip_marching_resource_usage(uint32_t maxWidth, uint32_t maxHeight, uint32_t maxDepth,
                                            uint32_t maxSwathe, uint64_t meshMemory, const uint32_t alignment[3]);
/* Marching::generate, src/marching.cpp:745-824: mlsgpu_hip_marching_generate_batch (below) with one bucket.  Blocks until
 * the bucket is done (as the reference's does). */
int mlsgpu_hip_marching_generate(mlsgpu_marching *m, const mlsgpu_generator *generator,
                                 mlsgpu_output_fn output, void *outputUser,
                                 const uint32_t size[3], const uint32_t keyOffset[3]);
/* Folds a ScaleBiasFilter (src/mesh_filter.cpp:69-113) into vertex emission: with enabled != 0 every vertex
 * handed to the output functor is already fma(v, scale, bias), bit-identical to running mlsgpu_hip_scale_bias
 * on the mesh afterwards, without the extra pass over HBM.  The worker uses this for its scale/bias filter. */
int mlsgpu_hip_marching_set_vertex_transform(mlsgpu_marching *m, int enabled, float scale, float bx, float by, float bz);
/* Counters marching.overflow / marching.shipouts / marching.slices.nonempty (src/marching.cpp:342-377) and
 * work totals: out[0]=overflow out[1]=shipouts out[2]=nonempty swathes out[3]=occupied cells
 * out[4]=unwelded vertices out[5]=indices out[6]=welded vertices out[7]=external vertices. */
int mlsgpu_hip_marching_counters(const mlsgpu_marching *m, uint64_t out[8]);
/* Lookup tables (src/marching.cpp:109-252): count[256][2] u8, start[257][2] u16, data[8192] u8, key[2432][3] u32 */
int mlsgpu_hip_marching_tables(const mlsgpu_marching *m, uint8_t *count, uint16_t *start, uint8_t *data, uint32_t *key);
/* Marching::copySlice (src/marching.cpp:447-498) on an arbitrary field buffer. */
int mlsgpu_hip_marching_copy_slice(mlsgpu_marching *m, float *dField, uint64_t pitch, uint32_t src, uint32_t trg,
                                   uint32_t width, uint32_t height, uint32_t zStride);
/* kernels/marching.cl:295-326 stand-alone (test/test_marching.cpp:401-479). */
int mlsgpu_hip_compact_vertices(mlsgpu_ctx *ctx, float *dOutVertices, uint64_t *dOutKeys, uint32_t *dIndexRemap,
                                uint32_t *dFirstExternal, const uint32_t *dVertexUnique, const float *dInVertices4,
                                const uint64_t *dInKeys, uint64_t minExternalKey, uint64_t keyOffset, uint64_t n);

/* ---- mesh plumbing ---- */
/* MeshSizes::getHostBytes, src/mesh.h:75-80 */
uint64_t mlsgpu_hip_mesh_host_bytes(const mlsgpu_mesh *mesh);
/* enqueueReadMesh into a HostKeyMesh blob [extKeys u64][vertices 3xf32][triangles 3xu32]
 * (src/mesh.cpp:51-102).  hostBlob must be 8-byte aligned.  async != 0: caller synchronises. */
int mlsgpu_hip_mesh_read(mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh, void *hostBlob, int async);
/* Measurement aid (bench.py and the full-size tests check the meshes a timed pass produced without copying gigabytes
 * to the host): out[0..2] = for the vertex words, the triangle indices and the external keys (as 32-bit words) the
 * sum of word[i] * (2 i + 1) modulo 2^64.  Synchronises the stream. */
int mlsgpu_hip_mesh_checksum(mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh, uint64_t out[3]);
/* ScaleBiasFilter, src/mesh_filter.cpp:69-113 + kernels/scale_bias.cl:33-41: in place. */
int mlsgpu_hip_scale_bias(mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh, float scale, float bx, float by, float bz);

/* The MlsFunctor behind a generator made by mlsgpu_hip_mls_generator, or NULL for any other generator. */
mlsgpu_mls *mlsgpu_hip_mls_of_generator(const mlsgpu_generator *gen);
/* kernel variant, work counters and boundary limit of `src` for `dst` (same shape) */
int mlsgpu_hip_mls_copy_settings(mlsgpu_mls *dst, const mlsgpu_mls *src);
/* MlsFunctor::enqueue (mlsgpu_hip_mls_enqueue) for `count` buckets in ONE launch: functor k fills dFields[k] (pitches[k]
 * floats per row, fieldRows[k] rows -- NULL: unchecked) for swathes[k].  The functors share a context, the shape and the
 * kernel variant. */
int mlsgpu_hip_mls_enqueue_batch(mlsgpu_mls *const *mls, float *const *dFields, const uint64_t *pitches,
                                 const uint64_t *fieldRows, const mlsgpu_swathe *swathes, uint32_t count);

/* Output functor of a batch: as mlsgpu_output_fn, with the index of the bucket the mesh belongs to. */
typedef int (*mlsgpu_batch_output_fn)(void *user, uint32_t index, void *stream, const mlsgpu_mesh *mesh);
/* Marching::generate (src/marching.cpp:745-824) for `count` buckets in lock-step: marchings[k] (distinct objects of one
 * context) takes generators[k], sizes[3k..] and keyOffsets[3k..]; one set of launches with a bucket dimension, the swathe
 * totals and the welded counts of all buckets read back together.  A bucket's meshes do not depend on the buckets it shares
 * the launches with; they are delivered bucket by bucket in order.  A bucket whose swathe overflows the mesh memory is split
 * behind the shared launches; when a bucket needs several swathes (or MLSGPU_HIP_WELD=sort) the buckets of the call go
 * through the reference's swathe loop one at a time.  Blocks. */
int mlsgpu_hip_marching_generate_batch(mlsgpu_marching *const *marchings, const mlsgpu_generator *generators, uint32_t count,
                                       mlsgpu_batch_output_fn output, void *outputUser,
                                       const uint32_t *sizes, const uint32_t *keyOffsets);

/* ---- DeviceWorkerGroupBase::Worker (src/workers.cpp:207-286): tree + MlsFunctor + Marching + ScaleBias ---- */
typedef struct mlsgpu_worker_config
{
    uint64_t maxBucketSplats;
    uint32_t maxCells;          /* bucket side in cells; Marching gets maxCells+1 corners */
    uint64_t meshMemory;        /* 0: (maxCells^2 * 2) worst-case cells as src/mlsgpu_core.cpp:359-370 */
    uint32_t levels;            /* default 6 */
    uint32_t subsampling;       /* default 3 */
    float boundaryLimit;        /* default 1.0 */
    int shape;
    uint32_t maxSwathe;         /* 0: whole bucket depth (no 8192-row image limit on HBM buffers) */
    float gridSpacing;          /* ScaleBiasFilter::setScaleBias(fullGrid): spacing and getVertex(0,0,0) */
    float gridOrigin[3];
} mlsgpu_worker_config;

int mlsgpu_hip_worker_create(mlsgpu_ctx *ctx, const mlsgpu_worker_config *cfg, mlsgpu_worker **out);
void mlsgpu_hip_worker_destroy(mlsgpu_worker *w);
/* DeviceWorkerGroup::resourceUsage (src/workers.cpp:184-205) per worker with ONE lane, without the item pool; a worker that
 * takes `lanes` buckets in lock-step (mlsgpu_hip_worker_set_batch) holds _lanes(cfg, lanes) = lanes times that. */
uint64_t mlsgpu_hip_worker_resource_usage(const mlsgpu_worker_config *cfg);
uint64_t mlsgpu_hip_worker_resource_usage_lanes(const mlsgpu_worker_config *cfg, uint32_t lanes);
/* One SubItem of a WorkItem (src/workers.cpp:235-285): lowExtent = sub.grid.getExtent(i).first,
 * numVertices = sub.grid.numVertices(i).  dSplats is the WorkItem's device splat buffer.  It is
 * mlsgpu_hip_worker_process_batch (below) with one item. */
int mlsgpu_hip_worker_process(mlsgpu_worker *w, mlsgpu_splat *dSplats, uint64_t firstSplat, uint64_t numSplats,
                              const int32_t lowExtent[3], const uint32_t numVertices[3],
                              mlsgpu_output_fn output, void *outputUser);
/* DeviceWorkerGroup::SubItem (src/workers.h:161-168): one bucket of a WorkItem whose splats share a device buffer */
typedef struct mlsgpu_subitem
{
    uint64_t firstSplat, numSplats;
    int32_t lowExtent[3];
    uint32_t numVertices[3];
    mlsgpu_splat *dSplats;      /* NULL: the buffer given to the call (one WorkItem); else this bucket's own buffer, so that
                                 * the buckets of several small WorkItems can share a batch */
} mlsgpu_subitem;
/* Lanes: how many buckets the worker takes through the path in lock-step (1 .. MLSGPU_MAX_BATCH; default 1).  Each lane
 * owns a tree, a distance field, a lattice and a mesh arena (mlsgpu_hip_worker_resource_usage bytes per lane). */
int mlsgpu_hip_worker_set_batch(mlsgpu_worker *w, uint32_t lanes);
uint32_t mlsgpu_hip_worker_batch(const mlsgpu_worker *w);
/* How much shares one set of processCorners / marching launches inside a batch: as many consecutive buckets as hold the
 * corners of `buckets` buckets of the worker's full size, (maxCells + 1)^3 each -- `buckets` full-size ones, or more small
 * ones (0: the whole batch; default 2).  The octree build always spans all lanes.  Results do not depend on it. */
int mlsgpu_hip_worker_set_marching_group(mlsgpu_worker *w, uint32_t buckets);
uint32_t mlsgpu_hip_worker_marching_group(const mlsgpu_worker *w);
/* The loop over the SubItems of a WorkItem (src/workers.cpp:232-286) with the buckets taken `lanes` at a time: per group
 * one set of launches (octree build, processCorners, marching, each with a bucket dimension) and three host decisions.
 * A bucket's meshes do not depend on the buckets it shares launches with; `output` receives them bucket by bucket, in
 * order, with the bucket's index in `items`. */
int mlsgpu_hip_worker_process_batch(mlsgpu_worker *w, mlsgpu_splat *dSplats, const mlsgpu_subitem *items, uint32_t numItems,
                                    mlsgpu_batch_output_fn output, void *outputUser);
/* How many leading items of the last _process_batch call had delivered all their meshes when it returned (numItems after a
 * success; after a failure in mid-batch the rest of the items were not processed): src/workers.cpp:281-284 accounts per
 * bucket, and so can a caller of the batch.  mlsgpu_hip_worker_process counts as a call with one item: 1 or 0 after it. */
uint32_t mlsgpu_hip_worker_batch_completed(const mlsgpu_worker *w);
mlsgpu_tree *mlsgpu_hip_worker_lane_tree(mlsgpu_worker *w, uint32_t lane);
mlsgpu_marching *mlsgpu_hip_worker_lane_marching(mlsgpu_worker *w, uint32_t lane);
/* keep = 1: the worker does not modify dSplats (non-mutating tree build + raw-radius processCorners, see
 * mlsgpu_hip_tree_set_mutate): resident splats can be processed again without being restored.  Default 0. */
int mlsgpu_hip_worker_set_keep_splats(mlsgpu_worker *w, int keep);
mlsgpu_tree *mlsgpu_hip_worker_tree(mlsgpu_worker *w);
mlsgpu_mls *mlsgpu_hip_worker_mls(mlsgpu_worker *w);
mlsgpu_marching *mlsgpu_hip_worker_marching(mlsgpu_worker *w);

/* ---- bucket farm: CopyGroup + one DeviceWorkerGroup per GPU (src/workers.h:214-438, src/workers.cpp:87-418,
 *      assembled by SlaveWorkers, src/mlsgpu_core.cpp:704-741).  The caller plays BucketLoader: it hands over
 *      host splats of one bucket at a time (already in grid coordinates, see mlsgpu_hip_transform_splats);
 *      the farm batches buckets into device items of at most maxBucketSplats splats (CopyGroupBase::Worker::
 *      operator(), :377-418), stages each batch in pinned memory (two buffers, so filling the next batch
 *      overlaps the copy of the previous one), picks the device whose group can take an item and has the most
 *      unallocated splat capacity (flush(), :315-375), copies host->device on that device's copy stream and
 *      queues the item; `workersPerDevice` threads per GPU (--device-threads) process the buckets of an item
 *      with mlsgpu_hip_worker_process after waiting for the item's copy event. ---- */
typedef struct mlsgpu_farm mlsgpu_farm;
typedef struct mlsgpu_farm_config
{
    uint32_t numDevices;
    const int32_t *devices;        /* device ordinals; NULL = 0 .. numDevices-1 */
    uint32_t workersPerDevice;     /* default 1 */
    uint32_t spare;                /* extra device items per GPU beyond one per worker; default 1 */
    mlsgpu_worker_config worker;   /* maxBucketSplats is also the capacity of a device item */
    uint32_t copyThreads;          /* host threads (per copy side) mlsgpu_hip_farm_submit copies a bucket with; 0 = 4 */
    uint32_t stagingBuffers;       /* pinned staging buffers per copy side; 0 = the side's GPUs + 2 (the reference has one,
                                    * src/workers.cpp:367-372) */
} mlsgpu_farm_config;
/* Output functor with the chunk it belongs to (OutputGenerator, src/workers.h:225).  Called on the worker's
 * thread; `ctx` is that worker's context (use it for mlsgpu_hip_mesh_read).  NULL: meshes are only counted. */
typedef int (*mlsgpu_farm_output_fn)(void *user, int device, uint64_t chunkId, mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh);
int mlsgpu_hip_farm_create(const mlsgpu_farm_config *cfg, mlsgpu_farm_output_fn output, void *user, mlsgpu_farm **out);
void mlsgpu_hip_farm_destroy(mlsgpu_farm *farm);
/* CopyGroup::get + push for one bucket: copies the splats into the pinned staging buffer (flushing the
 * current batch first if they do not fit).  Blocks while every device item is in use. */
int mlsgpu_hip_farm_submit(mlsgpu_farm *farm, const mlsgpu_splat *hSplats, uint64_t numSplats,
                           const int32_t lowExtent[3], const uint32_t numVertices[3], uint64_t chunkId);
/* The two halves of submit for a loader that writes splats straight into the staging buffer, as the reference's
 * BucketLoader does (src/bucket_loader.cpp:56-128 fills the buffer CopyGroup::get returned, then pushes it):
 * acquire returns room for numSplats splats in pinned memory (flushing the current batch first if they do not
 * fit); push appends the bucket (at most the acquired number of splats) to the batch.  One acquire per push. */
int mlsgpu_hip_farm_acquire(mlsgpu_farm *farm, uint64_t numSplats, mlsgpu_splat **out);
int mlsgpu_hip_farm_push(mlsgpu_farm *farm, uint64_t numSplats, const int32_t lowExtent[3], const uint32_t numVertices[3],
                         uint64_t chunkId);
/* Flushes the last batch and waits until every queued bucket has been processed; reports the first error.  After an error
 * the farm refuses further buckets (queued ones are handed back unprocessed, their capacity restored): finish and destroy it. */
int mlsgpu_hip_farm_finish(mlsgpu_farm *farm);
/* out[0] buckets, [1] splats copied, [2] H2D bytes, [3] device items, [4] ship-outs, [5] vertices, [6] triangles,
 * [7] external vertices; per device d: out[8 + d] = buckets processed there (up to 16 devices). */
int mlsgpu_hip_farm_stats(mlsgpu_farm *farm, uint64_t out[24]);
/* ---- placement: where the farm's host threads and pinned memory live relative to the GPUs.  The reference places
 *      nothing (src/workers.cpp:320-351 chooses a device by free capacity only; its threads run where the scheduler puts
 *      them).  Here a GPU's NUMA node is read from sysfs (hipDeviceGetPCIBusId -> /sys/bus/pci/devices/<bdf>/numa_node) and
 *      the farm keeps one COPY SIDE per node that has one of its GPUs: a ring of pinned staging buffers allocated on that
 *      node, copy threads bound to it, feeding that node's GPUs; device worker threads are bound to their GPU's node, the
 *      read-back ring and the mesher thread to the first GPU's.  A batch is staged on the side of the GPU it would go to
 *      (most unallocated capacity) and sent to a GPU of that side -- to another side's only when none of its own can take
 *      an item.  On a one-node machine, or when sysfs does not say, there is one unbound side.  MLSGPU_HIP_SYSFS_ROOT
 *      (default /sys) and MLSGPU_HIP_DEVICE_NODES ("0,0,1,1") describe another machine to a test. ---- */
int mlsgpu_hip_device_node(int device);                                    /* -1: unknown */
int mlsgpu_hip_topology(uint32_t *numNodes, uint32_t cpusPerNode[16]);
/* the plan alone: deviceNodes[i] -> sideOfDevice[i] (sides numbered by first appearance), nodeOfSide[k], *numSides */
int mlsgpu_hip_plan_copy_sides(const int32_t *deviceNodes, uint32_t numDevices, uint32_t numNodes, int32_t *sideOfDevice,
                               int32_t *nodeOfSide, uint32_t *numSides);
/* test hook: copies through the farm's pool of copy threads compared with their sources (`rounds` copies of pseudo-random sizes up
 * to `bytes`; rounds = 0: ONE copy of exactly `bytes` bytes); returns the mismatches */
int mlsgpu_hip_test_copy_pool(uint32_t threads, uint32_t rounds, uint64_t bytes, int node);
int mlsgpu_hip_bind_thread_to_node(int node);                              /* the calling thread; 1 = bound, 0 = left alone */
/* out[0] copy sides, [1] node the read-back ring's memory is on, [2] NUMA nodes, [3] devices; per device d < 16:
 * out[4 + 3d] ordinal, [5 + 3d] node, [6 + 3d] side; per side k < 12: out[52 + 4k] node, [53 + 4k] node its staging memory
 * is on (queried), [54 + 4k] staging buffers, [55 + 4k] copy threads.  -1 = unknown / unused. */
int mlsgpu_hip_farm_placement(mlsgpu_farm *farm, int32_t out[100]);
/* The copy side's clock, seconds since the farm was created: out[0] filling staging (mlsgpu_hip_farm_submit's memcpy),
 * [1] waiting for a staging buffer, [2] waiting for a device item, [3] host-to-device copies (timed event pairs on the copy
 * streams), [4] first submit .. last flush, [5] copies, [6] batches sent to another side's GPU, [7] inside the runtime's
 * enqueue calls (event records + hipMemcpyAsync).  h2d_busy = [3] / [4]. */
int mlsgpu_hip_farm_copy_clock(mlsgpu_farm *farm, double out[8]);
/* The device workers' clock since the farm was created: out[0] sets of launches they ran (a batch of buckets in lock-step,
 * or one bucket), [1] buckets in them ([1] / [0] = buckets per set of launches), [2] seconds the workers waited for an item,
 * [3] seconds they spent processing, both summed over the workers. */
int mlsgpu_hip_farm_worker_clock(mlsgpu_farm *farm, double out[4]);
/* the same four figures for ONE device group (the `group`-th device of the configuration): what the greedy dispatch of
 * src/workers.cpp:320-351 gave that GPU and how long its workers sat without an item */
int mlsgpu_hip_farm_group_clock(mlsgpu_farm *farm, uint32_t group, double out[4]);
/* The most device items (DeviceWorkerGroup::WorkItem, src/workers.h:165-181) that were in flight at once since the farm
 * was created: taken from a group's pool by the copy side and not yet returned by a device worker. */
int mlsgpu_hip_farm_in_flight_max(mlsgpu_farm *farm, uint64_t *out);

/* HostKeyMesh, src/mesh.h:125-179: a ship-out in host memory -- keys of the EXTERNAL vertices only (they are the last
 * numVertices - numInternalVertices vertices), packed float xyz, uint32 index triplets. */
typedef struct mlsgpu_host_mesh
{
    const uint64_t *vertexKeys;
    const float *vertices;
    const uint32_t *triangles;
    uint64_t numVertices;
    uint64_t numTriangles;
    uint64_t numInternalVertices;
} mlsgpu_host_mesh;
/* MesherBase::InputFunctor (src/mesher.h:204-210) as the reference's device workers feed it: called on the farm's ONE
 * mesher thread (MesherGroup, src/workers.cpp:47-85), meshes in the order the ship-outs happened; `mesh` points into
 * the farm's pinned circular buffer and is valid until the functor returns. */
typedef int (*mlsgpu_farm_host_output_fn)(void *user, int device, uint64_t chunkId, const mlsgpu_host_mesh *mesh);
/* Routes every ship-out to the host as the reference does (OutputGeneratorBuilder::Functor, src/workers.h:488-509):
 * room in a pinned circular buffer of ringBytes (MesherGroup::meshBuffer, --mem-mesh; the worker blocks while it is
 * full), enqueueReadMesh (src/mesh.cpp:62-102) asynchronously on the worker's stream -- the worker goes on with the
 * next bucket -- and `fn` on the mesher thread once the reads have completed.  fn may be NULL (meshes are read back and
 * dropped).  Works for any number of GPUs: this is the path that brings buckets of different devices to ONE welder
 * (mlsgpu_hip_host_mesher_*).  Call before the first bucket is submitted; a device-side output functor given to
 * mlsgpu_hip_farm_create still runs first.  A ship-out larger than ringBytes is MLSGPU_ERR_LENGTH.  Calling it again
 * BETWEEN jobs (after mlsgpu_hip_farm_finish) hands the next job's meshes to another consumer; the ring keeps its size. */
int mlsgpu_hip_farm_set_host_output(mlsgpu_farm *farm, uint64_t ringBytes, mlsgpu_farm_host_output_fn fn, void *user);
/* The same route with the CONSUMER's memory instead of the ring: `landing(user, bytes, &ptr)` hands out room for one
 * ship-out (page-locked memory that stays the consumer's: mlsgpu_hip_host_mesher_farm_landing), the asynchronous read-back
 * lands there, and `fn` receives pointers into it which it may keep -- the reference's mesher also reads its
 * CircularBuffer allocation in place (src/workers.h:488-509, src/mesher.cpp:447-469) before it writes the block to its
 * temporary file; here the block never moves again.  No ship-out waits for room.  Same calling rules as
 * mlsgpu_hip_farm_set_host_output (before the first bucket, or between jobs); calling that one afterwards goes back to the
 * ring. */
typedef int (*mlsgpu_farm_landing_fn)(void *user, uint64_t bytes, void **out);
int mlsgpu_hip_farm_set_host_landing(mlsgpu_farm *farm, mlsgpu_farm_landing_fn landing, mlsgpu_farm_host_output_fn fn, void *user);
/* out[0] meshes read back, [1] bytes, [2] times a worker waited for ring space, [3] largest mesh in bytes */
int mlsgpu_hip_farm_host_stats(mlsgpu_farm *farm, uint64_t out[4]);
/* BucketLoader's world -> grid transform (src/bucket_loader.cpp:77-85, Grid::worldToVertex src/grid.cpp:99-106):
 * position = (position - reference) * (1/spacing) - lowExtent, radius *= 1/spacing.  Host-side, in place. */
void mlsgpu_hip_transform_splats(mlsgpu_splat *hSplats, uint64_t numSplats, const float reference[3], float spacing,
                                 const int32_t gridLowExtent[3]);

/* ---- bucketing of a cloud that is resident in HBM: Bucket::bucket, src/bucket.h:116-180 ---- */
typedef struct mlsgpu_grid          /* class Grid, src/grid.h: world = reference + spacing * vertex */
{
    float reference[3];
    float spacing;
    int32_t extents[6];             /* per axis [first, second): second - first cells, one more vertices */
} mlsgpu_grid;
typedef struct mlsgpu_bucket_params /* the arguments of Bucket::bucket, src/bucket.h:170-180 */
{
    uint64_t maxSplats;             /* --mem-bucket-splats / sizeof(Splat) */
    uint32_t maxCells;              /* side of a bucket in cells: (1 << (levels + subsampling - 1)) - 1 */
    uint32_t chunkCells;            /* output chunk alignment; 0 = none */
    uint32_t microCells;            /* requested microblock side; 0 = heuristic (chooseMicroSize) */
    uint64_t maxSplit;              /* maximum fan-out of one recursion level, >= 8 */
} mlsgpu_bucket_params;
typedef struct mlsgpu_bucket        /* what ProcessorType's callback receives, src/bucket.h:98-114 */
{
    int32_t extents[6];             /* the bucket's grid: same reference and spacing, these extents */
    uint64_t chunk[3];              /* Recursion::chunk */
    uint32_t depth;                 /* Recursion::depth */
    uint64_t numSplats;
    const uint32_t *dIds;           /* device: ids of the bucket's splats, ascending; valid during the callback -- or, for a
                                     * callback that reads them asynchronously, until the event it leaves in *consumed */
    const mlsgpu_splat *dSplats;    /* device: the array the ids index -- the caller's cloud (mlsgpu_hip_bucket) or the batch
                                     * of the streamed set that is resident during the callback (mlsgpu_hip_bucket_stream) */
    void **consumed;                /* out, optional: a hipEvent_t the callback recorded behind its last read of dIds (on any
                                     * stream of any device).  The bucketer orders whatever overwrites the list behind that
                                     * event ON THE GPU, so a callback that only ENQUEUES its gather (mlsgpu_hip_farm_submit_
                                     * device_async) need not wait for it: the leaves of a level are handed over back to back.
                                     * Left NULL: the list may be reused as soon as the callback returns.  The event must stay
                                     * alive until the next mlsgpu_hip_bucket call on this context has returned.  With
                                     * mlsgpu_hip_bucket_stream the resident batch (dSplats) is NOT covered: read it before
                                     * returning. */
} mlsgpu_bucket;
typedef int (*mlsgpu_bucket_fn)(void *user, mlsgpu_ctx *ctx, const mlsgpu_bucket *bucket);
/* Splits `region` into buckets of at most maxCells cells per side and maxSplats splats and calls fn for each non-empty
 * one, in the reference's order.  dSplats: all splats, world coordinates, on the device (non-finite ones are ignored
 * as by the reference's splat sets).  MLSGPU_ERR_DENSITY if a single cell holds more than maxSplats splats
 * (*cellSplats = how many).  The octree of counters of one level is dense here: at most 2^24 nodes. */
int mlsgpu_hip_bucket(mlsgpu_ctx *ctx, const mlsgpu_splat *dSplats, uint64_t numSplats, const mlsgpu_grid *region,
                      const mlsgpu_bucket_params *params, mlsgpu_bucket_fn fn, void *user, uint64_t *cellSplats);
/* FastBlobSet::makeBoundingGrid (src/splat_set_impl.h:770-811): the grid the reference reconstructs on -- reference 0,
 * extents floor(min(p - r) / spacing) rounded down to a multiple of bucketSize, and ceil(max(p + r) / spacing) -- from a
 * min / max reduction over the finite splats on the device.  MLSGPU_ERR_LENGTH (the message names the axis, *out is not
 * written) if an extent -- the lower one after the rounding -- does not fit int32, or is infinite because position -+ radius
 * of a finite splat overflowed: the reference throws there (src/grid.h:59-70). */
int mlsgpu_hip_bounding_grid(mlsgpu_ctx *ctx, const mlsgpu_splat *dSplats, uint64_t numSplats, float spacing,
                             uint32_t bucketSize, mlsgpu_grid *out);
/* BucketLoader (src/bucket_loader.cpp:77-85, Grid::worldToVertex src/grid.cpp:99-106) on the device:
 * dOut[i] = splat dIds[i] (or i if dIds is NULL) in the vertex coordinates of fullGrid:
 * (position - reference) / spacing - fullGrid.extents[first], radius / spacing.  dOut is what
 * mlsgpu_hip_worker_process takes, with lowExtent = bucket.extents[first] - fullGrid.extents[first] and
 * numVertices = bucket cells + 1 (the subGrid of src/bucket_loader.cpp:91-102). */
int mlsgpu_hip_bucket_load(mlsgpu_ctx *ctx, const mlsgpu_splat *dSplats, const uint32_t *dIds, uint64_t numSplats,
                           const mlsgpu_grid *fullGrid, mlsgpu_splat *dOut);

/* A bucket whose splats are already on GPU `device` (one of the farm's), e.g. from mlsgpu_hip_bucket's callback: the
 * device item is filled by mlsgpu_hip_bucket_load (gather of dIds + transform into fullGrid's vertex coordinates) --
 * no host copy.  Like a host bucket it goes to the device group with the most unallocated capacity
 * (src/workers.cpp:320-351), `device`'s own on a tie: for another GPU the gather runs on `device` and the item is
 * filled by a peer copy on the target's copy stream out of a ring of scratch buffers on `device` (gather -> copy -> reuse of
 * the slot are ordered by events on the GPUs), so a cloud resident on one GPU feeds all of them with several leaves in
 * flight.  The call returns when the gather has run: dIds may be reused, the peer copy and the bucket go on without the
 * caller.  lowExtent / numVertices as for mlsgpu_hip_worker_process.  */
int mlsgpu_hip_farm_submit_device(mlsgpu_farm *farm, int device, const mlsgpu_splat *dSplats, const uint32_t *dIds,
                                  uint64_t numSplats, const mlsgpu_grid *fullGrid, const int32_t lowExtent[3],
                                  const uint32_t numVertices[3], uint64_t chunkId);
/* The same without the wait: the call returns when the gather has been ENQUEUED; *consumed is a hipEvent_t (owned by the
 * farm, alive as long as it is) that fires when the gather has read dSplats and dIds -- what a bucketer's callback leaves in
 * mlsgpu_bucket::consumed.  A farm worker that finds several such buckets queued takes them through one set of launches
 * (mlsgpu_hip_farm_set_batch), which it rarely does when every leaf costs the feeder a round trip to a busy GPU. */
int mlsgpu_hip_farm_submit_device_async(mlsgpu_farm *farm, int device, const mlsgpu_splat *dSplats, const uint32_t *dIds,
                                        uint64_t numSplats, const mlsgpu_grid *fullGrid, const int32_t lowExtent[3],
                                        const uint32_t numVertices[3], uint64_t chunkId, void **consumed);

/* The buckets of a device item (the SubItems of a WorkItem) are taken through the path `lanes` at a time by
 * mlsgpu_hip_worker_process_batch instead of one by one (src/workers.cpp:232-286); 1 .. MLSGPU_MAX_BATCH, default 1.
 * Outputs are unchanged and still arrive bucket by bucket. */
int mlsgpu_hip_farm_set_batch(mlsgpu_farm *farm, uint32_t lanes);

/* ---- mesh sink for meshes that stay in HBM: OOCMesher's weld / components / prune / per-chunk output,
 *      src/mesher.h:203-330, src/mesher.cpp:220-852 ---- */
typedef struct mlsgpu_mesher mlsgpu_mesher;
int mlsgpu_hip_mesher_create(mlsgpu_ctx *ctx, mlsgpu_mesher **out);
void mlsgpu_hip_mesher_destroy(mlsgpu_mesher *mesher);
/* MesherBase::setPruneThreshold: components with fewer vertices than uint64(total * threshold) are dropped */
int mlsgpu_hip_mesher_set_prune_threshold(mlsgpu_mesher *mesher, double threshold);
/* on = 1: finalize runs beside other GPU work (the next job's buckets) and holds its union-find pass back to a quarter of
 * the wave slots -- no slower for surface-like meshes, and the other kernels keep their speed.  Default 0. */
int mlsgpu_hip_mesher_set_background(mlsgpu_mesher *mesher, int on);
/* Optional: room for this many vertices / triangles / external vertices in total (the arenas grow by reallocation
 * otherwise). */
int mlsgpu_hip_mesher_reserve(mlsgpu_mesher *mesher, uint64_t numVertices, uint64_t numTriangles, uint64_t numExternal);
/* MesherBase::InputFunctor for a DeviceKeyMesh: appends a copy of the mesh (device to device, on `from`'s stream).  On the
 * mesher's own device the call does not wait for the copy: it is ahead of whatever `from`'s stream does to the mesh next
 * (Marching reuses it), and the mesher waits for its pending appends before anything reads the arenas (finalize, boundary,
 * reset, a growing arena); a peer append synchronises.  Thread safe; `from` is the calling worker's context, on
 * the mesher's device or on ANOTHER GPU (then the append is a peer copy over the fabric: several GPUs' buckets welded
 * in one GPU's HBM).  Blocks may arrive in any order, chunk ids interleaved (OOCMesher::add indexes chunks[chunkId.gen]
 * and accepts any arrival order too); output chunks are in order of first arrival. */
int mlsgpu_hip_mesher_add(mlsgpu_mesher *mesher, mlsgpu_ctx *from, uint64_t chunkId, const mlsgpu_mesh *mesh);
/* a mlsgpu_farm_output_fn whose `user` is the mlsgpu_mesher: give it to mlsgpu_hip_farm_create and the farm's device
 * workers (of any of its GPUs) append their ship-outs to the device sink */
int mlsgpu_hip_mesher_farm_output(void *mesher, int device, uint64_t chunkId, mlsgpu_ctx *ctx, const mlsgpu_mesh *mesh);
/* Empties the mesher for the next job; arenas, scratch and outputs keep their capacity. */
int mlsgpu_hip_mesher_reset(mlsgpu_mesher *mesher);
/* Several meshers, one job (one process per GPU, every rank's meshes in its own HBM): the device sink's counterpart of
 * mlsgpu_hip_host_mesher_boundary / _boundary_read / _finalize_with below.  boundary() welds and labels what has been
 * added and exports every distinct external key with the (densely numbered) component that holds its vertex, and the
 * vertex / triangle count of every component; finalize_with() produces the output with the caller's verdict per component
 * in place of the prune rule.  No add between the two calls.  mlsgpu_amd/dist_sink.py merges the exports of all ranks in
 * one all-gather.
 * The export is reproducible and its numbering is part of the contract: the keys ascend; with the blocks taken in the
 * order (chunk by first arrival, arrival within the chunk) and their vertices numbered through, a component's root is the
 * smallest of its welded vertices (an external vertex is welded to the first vertex with its key in that order), and the
 * roots are numbered densely in ascending order of that vertex.  rootTriangles counts the triangles whose first index
 * lies in the component. */
int mlsgpu_hip_mesher_boundary(mlsgpu_mesher *mesher, uint64_t *numKeys, uint64_t *numRoots);
int mlsgpu_hip_mesher_boundary_read(mlsgpu_mesher *mesher, uint64_t *keys, uint32_t *keyRoot, uint64_t *rootVertices,
                                    uint64_t *rootTriangles);
int mlsgpu_hip_mesher_finalize_with(mlsgpu_mesher *mesher, const uint8_t *keepRoot, uint64_t numRoots, uint32_t *numChunks);
/* What MesherBase::write does before it writes files: weld by key, components, prune.  *numChunks = chunks that have
 * triangles (no output is produced for the others, src/mesher.cpp:820). */
int mlsgpu_hip_mesher_finalize(mlsgpu_mesher *mesher, uint32_t *numChunks);
/* Output chunk i (arrival order): packed float3 vertices and uint3 triangles on the device, indices relative to the
 * chunk's first vertex.  A vertex shared by two chunks is in both (externalRemap is per chunk, src/mesher.cpp:538-567).
 * Valid until the next finalize / destroy. */
int mlsgpu_hip_mesher_chunk(mlsgpu_mesher *mesher, uint32_t i, uint64_t *chunkId, uint64_t *numVertices, uint64_t *numTriangles,
                            const float **dVertices, const uint32_t **dTriangles);
/* getStatistics (src/mesher.cpp:491-536): out[0] welded vertices, [1] threshold, [2] components, [3] kept components,
 * [4] kept vertices (each welded vertex once), [5] kept triangles, [6] vertices added, [7] triangles added */
int mlsgpu_hip_mesher_stats(mlsgpu_mesher *mesher, uint64_t out[8]);

/* ---- topology report of a device-resident mesh: Manifold::isManifold (test/manifold.h:98-232) in its "count-all" form.
 *      The reference returns at the first defect; here every triangle and vertex is classified and counted, and the lowest
 *      index of each class is kept, from which the reference's verdict follows (firstKind / firstIndex).
 *      A triangle (i0, i1, i2) takes the first check that fails of i0 >= V, i0 == i1, i1 >= V, i1 == i2, i2 >= V, i2 == i0:
 *      a range failure is OUT_OF_RANGE, an equality DEGENERATE; such triangles take no further part.  The others give the
 *      half-edges a -> b, b -> c, c -> a.  A vertex is ISOLATED if no good triangle uses it, else DUPLICATED if it is an end of
 *      a half-edge that occurs more than once, else MIXED ("both in the interior and on the boundary") or TUNNEL ("tunnels
 *      between interior regions") as in the reference.  The mesh is manifold if all six counts are zero; only then are
 *      edges, numComponents, numBoundaries and eulerCharacteristic filled (0 otherwise, like the reference's Metadata). ---- */
#define MLSGPU_TOPO_OUT_OF_RANGE 0
#define MLSGPU_TOPO_DEGENERATE 1
#define MLSGPU_TOPO_ISOLATED 2
#define MLSGPU_TOPO_DUPLICATED 3
#define MLSGPU_TOPO_MIXED 4
#define MLSGPU_TOPO_TUNNEL 5
#define MLSGPU_TOPO_NONE 6
typedef struct mlsgpu_topology
{
    uint64_t numVertices, numTriangles;
    uint64_t count[6];      /* triangles (the first two) and vertices per class, indexed by MLSGPU_TOPO_* */
    uint64_t firstOf[6];    /* lowest triangle / vertex index of the class, UINT64_MAX if none */
    uint64_t duplicateEdges;/* half-edge records equal to their predecessor in (from, to) order */
    uint64_t boundaryEdges; /* distinct half-edges a -> b without b -> a */
    uint64_t edges;         /* (3 T + boundaryEdges) / 2 */
    uint64_t numComponents; /* connected components of the graph of vertices and edges */
    uint64_t numBoundaries; /* connected components of the graph of boundary edges (a vertex on several boundary runs joins
                             * them into one, test/manifold.h:84-87) */
    int64_t eulerCharacteristic;    /* V - edges + T */
    uint64_t firstIndex;    /* the reference's verdict: the lowest bad triangle if any, else the lowest classified vertex; */
    uint32_t firstKind;     /* its class, MLSGPU_TOPO_NONE (and firstIndex UINT64_MAX) for a manifold mesh */
    uint32_t manifold;      /* 1 or 0 */
} mlsgpu_topology;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_topology) == 176, "mlsgpu_topology is part of the ABI");
#else
typedef char mlsgpu_topology_size_is_176[sizeof(mlsgpu_topology) == 176 ? 1 : -1];
#endif
/* numTriangles triangles of three uint32 indices on ctx's device, numVertices vertices (no positions are needed).
 * MLSGPU_ERR_LENGTH if 3 * numTriangles or numVertices does not fit 32 bits.  No triangles: every vertex is isolated, and no
 * vertices either is manifold.  Scratch is allocated for the call and freed on return: 24 bytes per half-edge (the sort's
 * two sides), the sort's histogram, 18 bytes per vertex; MLSGPU_ERR_NOMEM if the device does not have it.  Blocks until the
 * report is there. */
int mlsgpu_hip_mesh_topology(mlsgpu_ctx *ctx, const uint32_t *dTriangles, uint64_t numTriangles, uint64_t numVertices,
                             mlsgpu_topology *out);
/* the same for output chunk i of a finalized device sink (the mesh of mlsgpu_hip_mesher_chunk), on the mesher's context */
int mlsgpu_hip_mesher_chunk_topology(mlsgpu_mesher *mesher, uint32_t i, mlsgpu_topology *out);
/* Host only: "" if the mesh is manifold, else one sentence for the first defect, in the reference's wording where the
 * report carries what it names (a DUPLICATED vertex stands for the reference's edge, and the offending index of a bad
 * triangle is not repeated).  At most len - 1 characters and a terminator are written to buf (which may be NULL); returns
 * the length of the whole sentence. */
uint64_t mlsgpu_hip_topology_reason(const mlsgpu_topology *t, char *buf, uint64_t len);

/* ---- vertex-clustering simplification of a device-resident mesh, so that a smaller mesh crosses the link.  The reference
 *      has no counterpart: its meshes leave the device whole (src/mesher.cpp:763-852) and are decimated by other tools.
 *      Deterministic: every float and double operation below is ONE correctly rounded IEEE operation (no contraction), and
 *      every sum is an integer sum.
 *      1. The cell of a vertex, per axis: c = floorf((p - origin) / cellSize) in float.  A vertex is invalid if a coordinate
 *         is not finite or a c lies outside [0, 2^21).  key = z << 42 | y << 21 | x.
 *      2. A cluster is the set of vertices with one key; clusters are ordered by ascending key.
 *      3. A cluster of one member keeps that member's position bit for bit.  Otherwise, per axis in double:
 *         d = p - origin, f = d / cellSize - c, q = llrint(f * 2^30); S = the int64 sum of q over the n members;
 *         mean = (S / n) * 2^-30; out = (float) (origin + (c + mean) * cellSize).
 *      4. Every index is replaced by its cluster.  A triangle with two equal clusters is collapsed and dropped; a survivor
 *         is rotated (which keeps its orientation) so that its smallest cluster comes first; survivors are ordered by
 *         (first, second, third) and of a run of equal triples one is kept -- (a, b, c) and (a, c, b) both stay.
 *      5. The output vertices are the clusters a kept triangle uses, numbered densely in key order; clusters nothing uses
 *         (and input vertices no triangle used) disappear.
 *      Clustering can make a mesh non-manifold: mlsgpu_hip_mesh_topology says whether it did, and mlsgpu_hip_mesh_repair
 *      makes it manifold again. ---- */
typedef struct mlsgpu_simplify_stats
{
    uint64_t inVertices, inTriangles;
    uint64_t outVertices, outTriangles;
    uint64_t collapsedTriangles;    /* two of the three clusters equal */
    uint64_t duplicateTriangles;    /* equal to a kept triangle: inTriangles = outTriangles + collapsed + duplicate */
} mlsgpu_simplify_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_simplify_stats) == 48, "mlsgpu_simplify_stats is part of the ABI");
#else
typedef char mlsgpu_simplify_stats_size_is_48[sizeof(mlsgpu_simplify_stats) == 48 ? 1 : -1];
#endif
/* numVertices packed float xyz and numTriangles uint32 index triples on ctx's device -> dOutVertices / dOutTriangles, which
 * the caller allocates with room for the INPUT's sizes (the result is never larger; its sizes are in *stats) and which must
 * not overlap the inputs.  MLSGPU_ERR_INVALID for a cellSize that is not finite or <= 0, a non-finite origin, an invalid
 * vertex or a triangle index >= numVertices (counted on the device: compared, never used as an address); nothing is promised
 * about the outputs then.  MLSGPU_ERR_LENGTH if 3 * numTriangles or numVertices does not fit 32 bits.  No vertices or no
 * triangles is not an error: the result is an empty mesh.  Scratch is allocated for the call and freed on return: 60 bytes
 * per vertex, 44 per triangle and the sorts' histogram; MLSGPU_ERR_NOMEM if the device does not have it.  Blocks until the
 * statistics are there (one more stream synchronisation inside: the largest cells size the sort). */
int mlsgpu_hip_mesh_simplify(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                             uint64_t numTriangles, const float origin[3], float cellSize, float *dOutVertices,
                             uint32_t *dOutTriangles, mlsgpu_simplify_stats *stats);
/* The same for every output chunk of a finalized device sink, on the mesher's context: each chunk is replaced by its
 * simplified mesh, the chunks are packed towards the front of the sink's output arrays, and mlsgpu_hip_mesher_chunk,
 * _chunk_topology and _write_ply then serve the simplified chunks (a chunk that lost all its triangles stays in the list,
 * empty).  *stats is the sum over the chunks; mlsgpu_hip_mesher_stats keeps reporting the finalize's numbers.  Chunks are
 * simplified INDEPENDENTLY: the vertices two chunks share (the seams between split output files) are clustered with each
 * chunk's own neighbours and are not matched afterwards.  MLSGPU_ERR_INVALID before finalize; may be called again (on the
 * simplified chunks).  After an error the sink's results are dropped: finalize again. */
int mlsgpu_hip_mesher_simplify(mlsgpu_mesher *mesher, const float origin[3], float cellSize, mlsgpu_simplify_stats *stats);

/* ---- the same clustering with every cluster's vertex at the minimiser of the plane-distance quadrics of the triangles that
 *      touch the cluster (Lindstrom's out-of-core simplification) instead of the mean, which chamfers every crease by a large
 *      fraction of a cell.  Steps 1, 2, 4 and 5 above apply word for word: on one input the output triangles, outVertices and
 *      the six statistics are mlsgpu_hip_mesh_simplify's.  Step 3 becomes the steps below.  Deterministic: every float and
 *      double operation is ONE correctly rounded IEEE operation (no contraction), and every sum is an int64 sum.
 *      3a. A cluster of one member keeps that member's position bit for bit.
 *      3b. Cell coordinates, per vertex and axis in double: g = ((double) p - (double) origin) / (double) cellSize; the
 *          centred offset of a vertex in its own cell is w = (g - (double) c) - 0.5, c of step 1.
 *      3c. The face vector of a triangle: n = (g1 - g0) x (g2 - g0), each component two products and one subtraction in the
 *          operation order of the normals' step 2.  Every vertex is valid, so |g| < 2^21 and n is finite.
 *      3d. M = the largest |component| of n over all triangles.  M == 0: no cluster has a quadric, every cluster of several
 *          members is `flat` (3f) and scaleExponent = 0.  Otherwise e is the integer with 2^e <= M < 2^(e + 1) (a subnormal M
 *          has its true exponent), E = 2 e + 1, so that every |n_i n_j| < 2^(E + 1); s = 60 - bitLength(numTriangles), the
 *          number of bits numTriangles takes; scaleExponent = E.
 *      3e. A triangle adds to the cluster of each of its corners, once per distinct cluster: corner k adds iff its cluster
 *          differs from the clusters of all corners j < k.  For the cluster of corner k, d = -((n.x*w.x + n.y*w.y) + n.z*w.z)
 *          with w the centred offset of corner k in its own cell (|d| <= 1.5 M, to the float cell's rounding); the six
 *          products n.x*n.x, n.x*n.y, n.x*n.z, n.y*n.y, n.y*n.z, n.z*n.z and the three d*n.x, d*n.y, d*n.z are each quantised
 *          as q = llrint(ldexp(x, s - E)) with ties to even and added to the cluster's int64 sums A[6] and b[3].
 *          |q| < 2^(s + 2), and fewer than 2^bitLength(numTriangles) triangles add to a cluster: every |sum| < 2^62, no input
 *          overflows.  The sums S[3] of step 3 are taken as they are there.
 *      3f. Per cluster of n > 1 members, in double: a_ij = (double) A_ij, b_i = (double) b_i, tr = (a00 + a11) + a22,
 *          m_k = (S_k / n) * 2^-30 - 0.5 (step 3's mean, centred).  tr == 0: the cluster is `flat`.  Otherwise
 *          mu = tr * 2^-10 -- a pull towards the mean that makes the system positive definite and leaves a plane's or a
 *          straight crease's vertex (rank 1 or 2) where the mean is along the free directions -- r_k = mu * m_k - b_k, and
 *          (A + mu I) x = r is solved by LDL^T without pivoting in exactly this order:
 *            d0 = a00 + mu; l10 = a01 / d0; l20 = a02 / d0;
 *            d1 = (a11 + mu) - l10 * a01; t = a12 - l20 * a01; l21 = t / d1;
 *            d2 = ((a22 + mu) - l20 * a02) - l21 * t;
 *            y0 = r0; y1 = r1 - l10 * y0; y2 = (r2 - l20 * y0) - l21 * y1;   z_k = y_k / d_k;
 *            x2 = z2; x1 = z1 - l21 * x2; x0 = (z0 - l10 * x1) - l20 * x2.
 *      3g. If an x_k is not finite or |x_k| > 0.5 the minimiser left the cluster's cell: the cluster is `escaped`.  Otherwise
 *          it is `solved`.
 *      3h. solved: out = (float) ((double) origin + (((double) c + 0.5) + x) * (double) cellSize) per axis.  flat and escaped:
 *          step 3's formula unchanged, (float) (origin + (c + mean) * cellSize) -- a mesh on which every cluster falls back
 *          is mlsgpu_hip_mesh_simplify's output bit for bit.
 *      The result depends neither on the schedule nor on the order of the triangles nor on the numbering of the vertices.  It
 *      does depend on which corner a triangle lists first, through the rounding of n and d only.  Scaling every coordinate, the
 *      origin and cellSize by one power of two scales the output exactly.  Limit: a triangle whose n_i n_j lie below
 *      2^-(s + 1) of the scale 2^(E + 1) quantises to nothing -- for a million triangles, 2^-41 of the largest squared face
 *      vector. ---- */
typedef struct mlsgpu_simplify_quadric_stats
{
    uint64_t inVertices, inTriangles;       /* these six: mlsgpu_simplify_stats, in its order */
    uint64_t outVertices, outTriangles;
    uint64_t collapsedTriangles;
    uint64_t duplicateTriangles;
    uint64_t solvedVertices;        /* output vertices at their quadric's minimiser */
    uint64_t flatVertices;          /* of several members, at the mean: no quadric (tr == 0) */
    uint64_t escapedVertices;       /* of several members, at the mean: the minimiser left the cell; outVertices = the */
                                    /* clusters of one member + solved + flat + escaped */
    int64_t scaleExponent;          /* E of step 3d */
} mlsgpu_simplify_quadric_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_simplify_quadric_stats) == 80, "mlsgpu_simplify_quadric_stats is part of the ABI");
#else
typedef char mlsgpu_simplify_quadric_stats_size_is_80[sizeof(mlsgpu_simplify_quadric_stats) == 80 ? 1 : -1];
#endif
/* Arguments, capacities (room for the INPUT's sizes), error codes and blocking as for mlsgpu_hip_mesh_simplify; the largest
 * face vector comes back with that call's one read-back in the middle, so there is no further synchronisation.  Scratch: 72
 * bytes per vertex more (nine int64 sums per possible cluster).  MLSGPU_HIP_SIMPLIFY_ACCUMULATE=plain takes the sums with up
 * to 27 atomics per triangle instead of combining the lanes of a wave that share a cluster first; the result is the same bit
 * for bit. */
int mlsgpu_hip_mesh_simplify_quadric(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                     uint64_t numTriangles, const float origin[3], float cellSize, float *dOutVertices,
                                     uint32_t *dOutTriangles, mlsgpu_simplify_quadric_stats *stats);
/* mlsgpu_hip_mesher_simplify with this placement: chunks INDEPENDENT, packed and served in the same way, the chunks' normals
 * dropped.  *stats is the sum over the chunks, scaleExponent the largest among the chunks that have one. */
int mlsgpu_hip_mesher_simplify_quadric(mlsgpu_mesher *mesher, const float origin[3], float cellSize,
                                       mlsgpu_simplify_quadric_stats *stats);

/* ---- area-weighted vertex normals of a device-resident mesh, so that what leaves the device can be shaded as it is.  The
 *      reference has no counterpart: its files carry positions and faces (src/fast_ply.cpp:443-521).  Computed from the
 *      FINISHED mesh (after prune, after a simplify, whose cluster means no MLS fit belongs to).  Deterministic: every float
 *      and double operation below is ONE correctly rounded IEEE operation (no contraction), and every sum is an integer sum.
 *      1. A triangle with an index >= V is counted in outOfRangeTriangles and takes no part (the index is compared, never
 *         used as an address).
 *      2. The face vector, in double: a = p1 - p0, b = p2 - p0 per axis on the float coordinates converted to double;
 *         c = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x), each component two products and one subtraction.
 *         If a component of c is not finite the triangle is counted in nonFiniteTriangles and takes no part.  A degenerate
 *         triangle has c = 0 and adds nothing.
 *      3. M = the largest |component| of c over the triangles that take part.  M == 0 (or no triangles): every normal is
 *         zero and scaleExponent = 0.  Otherwise e is the integer with 2^e <= M < 2^(e + 1) (frexp's exponent minus 1; a
 *         subnormal M has its true exponent), q = llrint(ldexp(component, 30 - e)) with ties to even -- |q| <= 2^31, so the
 *         int64 sums of fewer than 2^32 / 3 triangles cannot overflow -- and scaleExponent = e.
 *      4. S[v] = the int64 sum, per axis, of q over every corner of every participating triangle that is v.
 *      5. x = (double) S per axis, l2 = (x.x*x.x + x.y*x.y) + x.z*x.z, l = sqrt(l2), normal = (float) (x / l) per axis.
 *         l == 0: the normal is (0, 0, 0) and the vertex is counted in zeroNormals (vertices no triangle uses among them).
 *      6. Orientation: c = cross(p1 - p0, p2 - p0) is what the triangle order gives.  The pipeline's closed surfaces have
 *         positive signed volume (the field is negative inside), so these normals point OUT of the surface, the same way as
 *         the input splats' normals.
 *      Scaling every coordinate by a power of two leaves the normals bit for bit (and moves scaleExponent by twice the shift).
 *      Limits: a triangle whose face vector is below 2^-31 of the largest one's quantises to nothing (meshes here have
 *      triangles of one grid's size); the float coordinates of a finite mesh cannot overflow the double products. ---- */
typedef struct mlsgpu_normals_stats
{
    uint64_t numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t nonFiniteTriangles;    /* in range, but a component of the face vector is NaN or infinite */
    uint64_t zeroNormals;           /* vertices whose sum is (0, 0, 0): unused, or all their triangles degenerate / too small */
    int64_t scaleExponent;          /* e of step 3 */
} mlsgpu_normals_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_normals_stats) == 48, "mlsgpu_normals_stats is part of the ABI");
#else
typedef char mlsgpu_normals_stats_size_is_48[sizeof(mlsgpu_normals_stats) == 48 ? 1 : -1];
#endif
/* numVertices packed float xyz and numTriangles uint32 index triples on ctx's device -> dOutNormals, packed float xyz with
 * room for 3 * numVertices floats, which must not overlap the inputs.  MLSGPU_ERR_LENGTH if 3 * numTriangles or numVertices
 * does not fit 32 bits (checked before anything is allocated).  No vertices or no triangles is not an error.  Scratch is
 * allocated for the call and freed on return: 24 bytes per vertex (the int64 sums) and four counters; MLSGPU_ERR_NOMEM if
 * the device does not have it.  Blocks until the statistics are there: one stream synchronisation, at the end (M stays on
 * the device).  MLSGPU_HIP_NORMALS_ACCUMULATE=plain takes the sums with nine atomics per triangle instead of combining the
 * lanes of a wave that share a vertex first; the result is the same bit for bit. */
int mlsgpu_hip_mesh_normals(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                            uint64_t numTriangles, float *dOutNormals, mlsgpu_normals_stats *stats);
/* The normals of output chunk i of a finalized device sink (the mesh of mlsgpu_hip_mesher_chunk), on the mesher's context:
 * *dNormals is 3 floats per vertex of the chunk in an array the sink owns beside its vertices (allocated at the first call).
 * A chunk is computed at its first request and served again afterwards; finalize, finalize_with, reset and
 * mlsgpu_hip_mesher_simplify invalidate it, so normals requested after a simplify are those of the simplified chunk.
 * MLSGPU_ERR_INVALID before finalize.  Chunks are INDEPENDENT, as for simplify: a vertex two chunks share gets, in each
 * chunk, the sum over that chunk's triangles only -- the seams between split output files are not matched.  dNormals and
 * stats may each be NULL. */
int mlsgpu_hip_mesher_chunk_normals(mlsgpu_mesher *mesher, uint32_t i, const float **dNormals, mlsgpu_normals_stats *stats);

/* ---- Taubin lambda|mu smoothing of a device-resident mesh: the low-pass that takes out the terraces a simplify leaves and
 *      the facet noise of marching tetrahedra without shrinking the surface, before the mesh crosses the link.  The reference
 *      has no counterpart.  The triangles are left alone, so the topology report does not change.  Deterministic: every
 *      float and double operation below is ONE correctly rounded IEEE operation (no contraction), and every sum is an integer
 *      sum -- the output depends neither on the schedule nor on the order of the triangles, and renumbering the vertices
 *      permutes it bit for bit.
 *      1. A triangle with an index >= V is counted in outOfRangeTriangles (the index is compared, never used as an address);
 *         otherwise a triangle with two equal indices is counted in degenerateTriangles.  Neither takes part.
 *      2. The undirected edges {a, b} of the participating triangles are counted once each in numEdges.  An edge is a
 *         BOUNDARY edge (boundaryEdges) if exactly one triangle side uses it, a -> b and b -> a counted together (a side used
 *         twice in the same direction is no boundary).  A vertex on a boundary edge is a boundary vertex (boundaryVertices),
 *         a vertex on no edge is isolated (isolatedVertices).
 *      3. The neighbour set N(v): for an interior vertex every vertex it shares an edge with; for a boundary vertex the
 *         empty set under MLSGPU_SMOOTH_BOUNDARY_FIXED (it keeps its position bit for bit through every pass) and the
 *         vertices it shares a BOUNDARY edge with under MLSGPU_SMOOTH_BOUNDARY_CURVE.  k = |N(v)|; a vertex with k = 0
 *         never moves.
 *      4. M = the largest |coordinate| over all V input vertices.  M == 0 or V == 0: the output is the input and
 *         scaleExponent = 0.  Otherwise e is the integer with 2^e <= M < 2^(e + 1) (as for the normals), fixed for the whole
 *         call, and scaleExponent = e.
 *      5. One pass with factor f, F = (double) f: for every vertex with k > 0, per axis, on the positions p as the previous
 *         pass left them (Jacobi: all reads come before all writes):
 *           Q(x) = llrint(ldexp((double) x, 30 - e)), ties to even;  S = the int64 sum of Q(p_n) over n in N(v), modulo 2^64;
 *           D = S - k * Q(p_v), modulo 2^64;  d = ldexp((double) D / (double) k, e - 30);  out = (float) ((double) p_v + F * d).
 *         The vertex's own position is never quantised: a vertex whose neighbours balance keeps its bits.
 *      6. An iteration is a lambda pass followed, if mu != 0, by a mu pass.  passes = iterations * (mu != 0 ? 2 : 1), also
 *         where step 4 makes them the identity.  iterations = 0 copies the input; the counts of steps 1-2 are still filled.
 *      7. maxMove = the largest |(double) out - (double) in| over vertices and axes; maxCoordinate = the largest |coordinate|
 *         of the input and of every pass's output.  If maxCoordinate is not finite or exceeds 2^(e + 21) the call has
 *         DIVERGED: MLSGPU_ERR_INVALID, and nothing is promised about the outputs.  (Values are clamped before they become
 *         integers, so every conversion is defined, and no address ever depends on a coordinate.)
 *      Scaling every coordinate by 2^s scales the output exactly and moves scaleExponent by s (away from the subnormals). ---- */
#define MLSGPU_SMOOTH_BOUNDARY_FIXED 0
#define MLSGPU_SMOOTH_BOUNDARY_CURVE 1
typedef struct mlsgpu_smooth_stats
{
    uint64_t numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t degenerateTriangles;   /* in range, two indices equal */
    uint64_t numEdges;              /* undirected, of the participating triangles */
    uint64_t boundaryEdges;         /* used by exactly one triangle side */
    uint64_t boundaryVertices;      /* on a boundary edge */
    uint64_t isolatedVertices;      /* on no edge */
    uint64_t passes;                /* step 6 */
    int64_t scaleExponent;          /* e of step 4 */
    double maxMove, maxCoordinate;  /* step 7 */
} mlsgpu_smooth_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_smooth_stats) == 96, "mlsgpu_smooth_stats is part of the ABI");
#else
typedef char mlsgpu_smooth_stats_size_is_96[sizeof(mlsgpu_smooth_stats) == 96 ? 1 : -1];
#endif
/* numVertices packed float xyz and numTriangles uint32 index triples on ctx's device -> dOutVertices, packed float xyz with
 * room for 3 * numVertices floats, which may be exactly dVertices (in place); any other overlap is not allowed.
 * MLSGPU_ERR_INVALID, before anything touches the device, unless lambda and mu are finite, 0 < lambda <= 1, -1 <= mu <= 0,
 * boundary is one of the two values above and stats is not NULL; MLSGPU_ERR_INVALID for a coordinate that is not finite
 * (counted on the device) and for a call that diverged (step 7).  MLSGPU_ERR_LENGTH, before anything is allocated, unless
 * numVertices < 2^32 and 6 * numTriangles < 2^32: both directions of every triangle side are sorted, and the sort's values
 * are 32-bit.  No vertices or no triangles is not an error.  Scratch is allocated for the call and freed on return: 144 bytes
 * per triangle (six directed edge records: the two sides of the sort's 64-bit keys and 32-bit values; the neighbour lists
 * reuse the side the sort leaves free), 41 bytes per vertex (two working position arrays of 16-byte rows, the neighbour
 * run 8, a boundary flag 1), the sort's histogram and the scan's tile sums; MLSGPU_ERR_NOMEM if the device does not have it.
 * Blocks until the statistics are there: one stream synchronisation behind the adjacency build (the input's extent sizes the
 * fixed point), one at the end.  MLSGPU_HIP_SMOOTH_PASS=serial walks a neighbour list one entry after the other instead of
 * four entries a round with their loads issued together; the result is the same bit for bit. */
int mlsgpu_hip_mesh_smooth(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                           uint64_t numTriangles, uint32_t iterations, float lambda, float mu, uint32_t boundary,
                           float *dOutVertices, mlsgpu_smooth_stats *stats);
/* The same for every output chunk of a finalized device sink, on the mesher's context: each chunk's vertices are smoothed
 * where they lie, in place; triangles and chunk layout are untouched, and the chunks' normals are dropped, so normals
 * requested afterwards are those of the smoothed chunk.  *stats: the counts summed over the chunks, passes as for one chunk,
 * scaleExponent, maxMove and maxCoordinate the maxima over the chunks.  Chunks are smoothed INDEPENDENTLY, as for simplify
 * and normals.  Under MLSGPU_SMOOTH_BOUNDARY_FIXED a vertex two chunks share lies on the boundary of each and so keeps its
 * bits in both: the seams between split output files stay closed.  (Under _CURVE it moves with each chunk's own boundary
 * neighbours, and the seams may open.)  MLSGPU_ERR_INVALID before finalize; may be called again, and after a simplify.  After
 * an error the sink's results are dropped: finalize again. */
int mlsgpu_hip_mesher_smooth(mlsgpu_mesher *mesher, uint32_t iterations, float lambda, float mu, uint32_t boundary,
                             mlsgpu_smooth_stats *stats);

/* ---- Delaunay edge flips of a device-resident mesh, with a triangle quality report: marching tetrahedra leaves needles and
 *      caps wherever the surface passes close to a lattice vertex, and a cluster simplify adds its own; flipping an interior
 *      edge whose two opposite angles sum to more than pi (the intrinsic Delaunay criterion) takes them out by changing the
 *      connectivity only.  Vertices keep their bits, boundary edges are never flipped (the seams between output chunks stay
 *      closed), and the topology report of the result is the input's.  The reference has no counterpart.  Deterministic:
 *      every floating-point operation below is ONE correctly rounded IEEE double operation on exactly converted floats (no
 *      contraction), in the order written, and every statistic is a count, a minimum or a maximum -- the output depends
 *      neither on the schedule nor on the order of the triangles.  For vectors u, v of doubles
 *        u - v = (ux - vx, uy - vy, uz - vz);  dot(u, v) = (ux * vx + uy * vy) + uz * vz;
 *        cross(u, v) = (uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx);  face(p, q, r) = cross(q - p, r - p).
 *      1. A triangle with an index >= V is counted in outOfRangeTriangles (the index is compared, never used as an address);
 *         otherwise a triangle with two equal indices is counted in degenerateTriangles.  Neither takes part, in any round:
 *         their rows keep their bits.  (A flip never makes a participating triangle degenerate: step 3 and guard (i).)
 *      2. The undirected edges {a, b} of the participating triangles are counted once each in numEdges.
 *      3. An edge {a, b}, a < b, is INTERIOR REGULAR (interiorEdges) if exactly one triangle side is a -> b and exactly one is
 *         b -> a, with T1 = (a, b, c) the triangle that holds a -> b and T2 = (b, a, d) the one that holds b -> a (each up to
 *         rotation), and c != d.
 *      4. Priority.  cot(p; q, r) = dot(q - p, r - p) / sqrt(dot(x, x)) with x = cross(q - p, r - p).
 *         P = -(cot(c; a, b) + cot(d; b, a)).  The edge is NON-DELAUNAY if P > minGain; a NaN P never is, +infinity is (a
 *         zero-area cap has it).  P is a ratio: scaling all coordinates by a power of two changes no output bit (as long
 *         as nothing leaves the doubles' normal range).
 *      5. Guards.  With n1 = face(a, b, c), n2 = face(b, a, d), N = n1 + n2, m1 = face(a, d, c), m2 = face(b, c, d), a
 *         non-Delaunay edge is BLOCKED if
 *           (i)   c -> d or d -> c is a side of a participating triangle, or
 *           (ii)  dot(n1, n2) >= (minCos * sqrt(dot(n1, n1))) * sqrt(dot(n2, n2)) is false, or
 *           (iii) dot(m1, N) > 0 && dot(m2, N) > 0 is false (the quad is not convex, or the flip would fold it),
 *         and a CANDIDATE otherwise.
 *      6. The choice of a round.  A candidate WINS if at each of its four vertices a, b, c, d it is the best of all candidates
 *         that have that vertex among their four: the larger P wins, among equal P the smaller key a << bitLength(V) | b.
 *         (bitLength(V) = the number of bits of V: 0 for 0, 3 for 4.)  Winners have disjoint vertex sets: no two share a
 *         triangle or create the same edge, none invalidates another's guard (i), and their order does not matter.  The best
 *         candidate of the mesh always wins: a round without a winner is a round without a candidate.
 *      7. Rewrite.  For every winner the row of T1 becomes (a, d, c) and the row of T2 becomes (b, c, d).  Nothing else is
 *         written.
 *      8. Rounds.  The mesh is classified (steps 3-5); then, while fewer than maxRounds rounds have run: a round chooses and
 *         rewrites (rounds counts it); if it had no winner, converged = 1 and the rounds end; otherwise its winners are added
 *         to flips and the mesh is classified again.  maxRounds is a required cap: near-cocircular quads can alternate under
 *         rounding.  maxRounds = 0 is a pure report (rounds = 0, converged = 0) and the output is a copy of the input.
 *         A mesh in which no triangle takes part -- none at all, or V == 0 -- has no candidate: rounds = converged = 1 unless
 *         maxRounds = 0.
 *         nonDelaunayBefore is the first classification's number of non-Delaunay edges; nonDelaunayAfter and blockedAfter
 *         are the last one's non-Delaunay and blocked edges -- those of the output mesh.  After convergence they are equal.
 *      9. Quality.  For a participating triangle (p, q, r), with x = face(p, q, r), u = q - p, v = r - q, w = p - r:
 *           q = (C * sqrt(dot(x, x))) / ((dot(u, u) + dot(v, v)) + dot(w, w)),  C = 3.4641016151377544 (the double at 2 sqrt 3);
 *         q = 0 where the denominator is 0 or q is NaN.  q is 1 for an equilateral triangle and 0 for one without area.
 *         quality*[min(15, floor(16 q))] counts the triangles, minQuality* is the smallest q (0 if no triangle takes part);
 *         *Before of the input, *After of the output. ---- */
typedef struct mlsgpu_flip_stats
{
    uint64_t numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t degenerateTriangles;   /* in range, two indices equal */
    uint64_t numEdges;              /* undirected, of the participating triangles */
    uint64_t interiorEdges;         /* step 3 */
    uint64_t rounds, flips, converged;                      /* step 8 */
    uint64_t nonDelaunayBefore, nonDelaunayAfter, blockedAfter;
    double minQualityBefore, minQualityAfter;               /* step 9 */
    uint64_t qualityBefore[16], qualityAfter[16];
} mlsgpu_flip_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_flip_stats) == 368, "mlsgpu_flip_stats is part of the ABI");
#else
typedef char mlsgpu_flip_stats_size_is_368[sizeof(mlsgpu_flip_stats) == 368 ? 1 : -1];
#endif
/* numVertices packed float xyz and numTriangles uint32 index triples on ctx's device -> dOutTriangles, uint32 triples with
 * room for 3 * numTriangles words, which may be exactly dTriangles (in place); any other overlap is not allowed.  Triangle t
 * of the output is triangle t of the input, flipped or not.  MLSGPU_ERR_INVALID, before anything touches the device, unless
 * minGain is finite and >= 0, -1 <= minCos <= 1 and stats is not NULL; MLSGPU_ERR_INVALID for a coordinate that is not finite
 * (counted on the device; nothing is promised about the output then).  MLSGPU_ERR_LENGTH, before anything is allocated,
 * unless numVertices < 2^32 and 3 * numTriangles < 2^32: the sides of every triangle are sorted, and the sort's values are
 * 32-bit.  No vertices or no triangles is not an error.  Scratch is allocated for the call and freed on return: 96 bytes per
 * triangle (three directed side records: the two sides of the sort's 64-bit keys and 32-bit values 72 -- the side the sort
 * leaves free holds each record's priority and partner -- and the two opposite vertices 24), 24 bytes per vertex (the best
 * priority, the best key, and where the sides that leave the vertex lie), and the sort's histogram; MLSGPU_ERR_NOMEM if the
 * device does not have it.  Blocks until the statistics are there: one stream synchronisation per classification, to read
 * its counts -- rounds + 1 of them, or rounds where the last round had no winner -- and one at the end. */
int mlsgpu_hip_mesh_flip_edges(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                               uint64_t numTriangles, uint32_t maxRounds, double minGain, double minCos,
                               uint32_t *dOutTriangles, mlsgpu_flip_stats *stats);
/* The same for every output chunk of a finalized device sink, on the mesher's context, after any fill / simplify / repair /
 * smooth: each chunk's triangles are flipped where they lie, in place; vertices and chunk layout are untouched, and the
 * chunks' normals are dropped, so normals requested afterwards are those of the flipped chunk.  Chunks are flipped
 * INDEPENDENTLY; an edge two chunks share is a boundary edge of each and is never flipped, so the seams stay closed.
 * *stats: the counts and histograms summed over the chunks, rounds the largest, converged the AND over the chunks that have
 * triangles (without one: as for a mesh without triangles), the two minima the minima over them.  MLSGPU_ERR_INVALID before
 * finalize and for the parameters mlsgpu_hip_mesh_flip_edges refuses (no results are lost then); may be called again.  After
 * any other error the sink's results are dropped: finalize again. */
int mlsgpu_hip_mesher_flip_edges(mlsgpu_mesher *mesher, uint32_t maxRounds, double minGain, double minCos,
                                 mlsgpu_flip_stats *stats);

/* ---- short-edge collapse of a device-resident mesh, with the flips' triangle quality report: marching tetrahedra's worst
 *      slivers have a short edge -- two vertices almost on top of each other where the surface passes close to a lattice
 *      vertex --, which no flip improves.  Collapsing an interior edge of at most maxLength takes the needle out where it is:
 *      one vertex and two triangles go, a vertex moves by at most maxLength / 2, and everything else keeps its bits.  The
 *      reference has no counterpart.  Deterministic in the flips' sense: every floating-point operation below is ONE
 *      correctly rounded IEEE double operation on exactly converted floats (no contraction), in the order written, every
 *      statistic is a count, a minimum or a maximum, and the output depends neither on the schedule nor on the order of the
 *      triangles or of a triangle's corners (only q of step 11 is taken in a row's own order, as for the flips).  u - v, dot,
 *      cross and face are those of the flips.  T = maxLength * maxLength.
 *      1. Participation is step 1 of the flips: a triangle with an index >= V is counted in outOfRangeTriangles, otherwise one
 *         with two equal indices in degenerateTriangles (both of the input), and neither takes part; unlike there, they are
 *         not part of the output, which is renumbered.
 *      2. The SIDES are the directed sides of the participating triangles.  A vertex is FIXED if a side that leaves it or
 *         arrives at it occurs more than once or has no reverse: every boundary vertex -- and with them every seam between
 *         output chunks -- and the ends of irregular edges.  numEdges, interiorEdges (step 3) and fixedVertices are those of
 *         the first classification.
 *      3. An edge {a, b}, a < b, is INTERIOR REGULAR as in step 3 of the flips, with T1 = (a, b, c), T2 = (b, a, d), c != d.
 *      4. L2 = dot(pb - pa, pb - pa).  The edge is SHORT if L2 <= T (never for a NaN; an edge of length zero is short even at
 *         maxLength 0).  minLengthSq* is the smallest L2 of the interior regular edges, +infinity if there is none.
 *      5. Survivor.  If exactly one end is fixed, it survives with the bits of its position and the other end is removed.  If
 *         neither is, a survives and b is removed, and the new position is, per coordinate,
 *         (float) (((double) pa + (double) pb) * 0.5).  (Both fixed: guard (i).)
 *      6. Guards.  N(x) = the other vertices of the participating triangles that hold x.  A short edge is BLOCKED if
 *           (i)   both ends are fixed, or
 *           (ii)  more than MLSGPU_COLLAPSE_MAX_VALENCE participating triangles hold a, or more than that hold b (the bound
 *                 on what one thread walks; marching's valences are far below it), or
 *           (iii) N(a) and N(b) have a vertex other than c and d in common (the link condition), or
 *           (iv)  c -> d or d -> c is a side (the link condition's edge part, conservatively: it blocks the tetrahedron), or
 *           (v)   a participating triangle other than T1 and T2 that holds x = a or x = b fails the fold test: rotated to
 *                 (x, q, r), with n = face(px, pq, pr) and n' = face(p', pq, pr), p' the double of the new position, it
 *                 fails if dot(n, n) != 0 and
 *                 dot(n, n') > 0 && dot(n, n') >= (minCos * sqrt(dot(n, n))) * sqrt(dot(n', n')) is false,
 *         and a CANDIDATE otherwise.
 *      7. The choice of a round.  With S = {a, b} + N(a) + N(b), a candidate WINS if at every vertex of its S it is the best of
 *         all candidates that have that vertex in their S: the smaller L2 wins, among equal L2 the smaller key
 *         a << bitLength(V) | b, in the input's vertex numbers.  Winners have disjoint S: no triangle is near two of them,
 *         none changes another's guards, and their order does not matter.  The best candidate of the mesh always wins: a
 *         round without a winner is a round without a candidate.
 *      8. Rewrite.  For every winner the removed vertex becomes the survivor in every triangle that holds it -- T1 and T2
 *         then name the survivor twice and take no part any more -- and the survivor gets its position.
 *      9. Rounds, as step 8 of the flips: the mesh is classified (steps 1-6, on the rewritten rows and positions); then,
 *         while fewer than maxRounds rounds have run: a round chooses and rewrites (rounds counts it); if it had no winner,
 *         converged = 1 and the rounds end; otherwise its winners are added to collapses and the mesh is classified again.
 *         maxRounds = 0 is a pure report.  A mesh in which no triangle takes part has rounds = converged = 1 unless
 *         maxRounds = 0.  shortBefore is the first classification's number of short edges; shortAfter and blockedAfter are
 *         the last one's short and blocked edges -- those of the output mesh.  After convergence they are equal.
 *     10. Output.  The vertices that a participating triangle still uses, in ascending input order, each with the bits it
 *         ended with (outVertices; unusedVertices counts the others, removed or never used); the participating triangles in
 *         input order with their corners renumbered (outTriangles); dOutSource, if not NULL, gets every output vertex's
 *         input index.
 *     11. Quality: q of step 9 of the flips, *Before of the input, *After of the output.
 *      What follows: an input that mlsgpu_hip_mesh_topology calls manifold gives an output with the same manifold flag,
 *      components, boundaries, boundary edges and Euler characteristic; fixed vertices keep their order and their bits; a mesh
 *      without a short edge, a defect or an unused vertex comes back bit for bit; collapsing a converged output again makes
 *      no collapse; scaling the coordinates and maxLength by a power of two scales the output and changes no count (as long
 *      as nothing leaves the floats' and doubles' normal range). ---- */
#define MLSGPU_COLLAPSE_MAX_VALENCE 64u
typedef struct mlsgpu_collapse_stats
{
    uint64_t numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t degenerateTriangles;   /* in range, two indices equal */
    uint64_t numEdges;              /* undirected, of the participating triangles */
    uint64_t interiorEdges;         /* step 3 */
    uint64_t fixedVertices;         /* step 2 */
    uint64_t rounds, collapses, converged;                  /* step 9 */
    uint64_t shortBefore, shortAfter, blockedAfter;
    uint64_t unusedVertices, outVertices, outTriangles;     /* step 10 */
    double minQualityBefore, minQualityAfter;               /* step 11 */
    double minLengthSqBefore, minLengthSqAfter;             /* step 4 */
    uint64_t qualityBefore[16], qualityAfter[16];
} mlsgpu_collapse_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_collapse_stats) == 416, "mlsgpu_collapse_stats is part of the ABI");
#else
typedef char mlsgpu_collapse_stats_size_is_416[sizeof(mlsgpu_collapse_stats) == 416 ? 1 : -1];
#endif
/* numVertices packed float xyz and numTriangles uint32 index triples on ctx's device -> dOutVertices / dOutTriangles (and
 * dOutSource, uint32 per output vertex, or NULL), with room for capVertices / capTriangles rows; no overlap with the inputs,
 * which are left alone.  The capacity rule and the size query are mlsgpu_hip_mesh_repair's: MLSGPU_ERR_LENGTH, with *stats
 * complete, if a capacity is below outVertices / outTriangles -- NULL outputs with zero capacities ask for the sizes (and
 * come back MLSGPU_OK if the result is empty).  MLSGPU_ERR_INVALID, before anything touches the device, unless maxLength is
 * finite and >= 0, 0 <= minCos <= 1 and stats is not NULL; MLSGPU_ERR_INVALID for a coordinate that is not finite (counted on
 * the device).  MLSGPU_ERR_LENGTH, before anything is allocated, unless numVertices < 2^32 and 3 * numTriangles < 2^32.  No
 * vertices or no triangles is not an error.  Scratch is allocated for the call and freed on return: 96 bytes per triangle
 * (three directed side records: the two sides of the sort's 64-bit keys and 32-bit values 72 -- the side the sort leaves free
 * holds a candidate's L2 --, each side's third vertex 12, the row's working copy 12), 44 bytes per vertex (the best L2, the
 * best key, where the sides that leave the vertex lie, the fixed flag, the position's working copy, the output number), the
 * sort's histogram and the scans' tile sums; MLSGPU_ERR_NOMEM if the device does not have it.  Blocks until the statistics
 * are there: one stream synchronisation per classification -- rounds + 1 of them, or rounds where the last round had no
 * winner -- one for the sizes and one behind the output. */
int mlsgpu_hip_mesh_collapse_edges(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                   uint64_t numTriangles, uint32_t maxRounds, double maxLength, double minCos,
                                   float *dOutVertices, uint64_t capVertices, uint32_t *dOutTriangles, uint64_t capTriangles,
                                   uint32_t *dOutSource, mlsgpu_collapse_stats *stats);
/* The same for every output chunk of a finalized device sink, on the mesher's context, after any fill / simplify / repair /
 * smooth / flip, by the route of mlsgpu_hip_mesher_repair: every chunk is sized first and then collapsed into new arrays,
 * each chunk behind the one before, and the new generation takes the old one's place only when all chunks are done -- an
 * error leaves the results as they were.  The chunks' normals are dropped.  Chunks are collapsed INDEPENDENTLY: a vertex two
 * chunks share lies on the boundary of each, so it is fixed in both and the seams stay closed bit for bit.  *stats: the counts
 * and histograms summed over the chunks, rounds the largest, converged the AND over the chunks that have triangles (without
 * one: as for a mesh without triangles), the four minima the minima over them.  MLSGPU_ERR_INVALID before finalize and for
 * the parameters mlsgpu_hip_mesh_collapse_edges refuses; may be called again. */
int mlsgpu_hip_mesher_collapse_edges(mlsgpu_mesher *mesher, uint32_t maxRounds, double maxLength, double minCos,
                                     mlsgpu_collapse_stats *stats);

/* ---- long-edge split of a device-resident mesh, with the flips' triangle quality report: the refine step next to collapse,
 *      flip and smooth.  A fan that caps a hole has spokes as long as the hole's radius and no vertex inside to flip or
 *      smooth with, and a simplify leaves edges of its cell size; halving every edge above maxLength, longest first, evens
 *      the sampling out and leaves the surface where it was, piecewise.  The reference has no counterpart.  Deterministic in
 *      the flips' sense: every floating-point operation below is ONE correctly rounded IEEE double operation on exactly
 *      converted floats (no contraction), in the order written, every statistic is a count, a minimum or a maximum, and the
 *      output depends neither on the schedule nor -- up to the order of its rows -- on the order of the triangles or of a
 *      triangle's corners.  u - v, dot, cross, face and q are those of the flips.  T = maxLength * maxLength.
 *      1. Participation is step 1 of the flips, decided once on the input: outOfRangeTriangles, degenerateTriangles.  A row
 *         that takes no part keeps its bits and its place in the output, as in the hole filling.
 *      2. The SIDES are the directed sides of the participating triangles.  An undirected edge {a, b}, a < b, is INTERIOR
 *         REGULAR as in step 3 of the flips (exactly one side a -> b, exactly one b -> a, c != d), BOUNDARY if exactly one
 *         side names it in either direction, and IRREGULAR otherwise.  numEdges, interiorEdges and boundaryEdges are those of
 *         the first classification.
 *      3. L2 = dot(pb - pa, pb - pa): a sum of squares in a fixed axis order, the same whichever end is called a.  The edge is
 *         LONG if L2 > T (never for a NaN).  maxLengthSq* is the largest L2 of all edges, 0 if there is none.
 *      4. A long edge is SPLITTABLE if it is interior regular or boundary and its two ends are not both pinned, and BLOCKED
 *         otherwise.  dPinned is NULL or one byte per INPUT vertex (not zero: pinned); a vertex that a split made is never
 *         pinned.
 *      5. Order within a triangle: side x comes before side y if L2x > L2y, or if they are equal and x has the smaller
 *         (lo, hi) pair of vertex numbers.  A triangle's three sides have three different pairs: every participating triangle
 *         has exactly one FIRST side.
 *      6. A splittable edge is a CANDIDATE if it is the first side of every triangle that holds it (one for a boundary edge,
 *         two for an interior one); blocked and short sides are compared like any other.  This is Rivara's longest-edge
 *         bisection.  Two candidates never share a triangle, so a round needs no arbitration and the order of its splits does
 *         not matter.  A triangle whose first side is blocked is frozen, and so are the long edges behind it.  The longest
 *         splittable long edge that is first in its triangles always is a candidate: a round without one is the end.
 *      7. A round, on V_r vertices and T_r rows.  The candidates are numbered j = 0, 1, ... in ascending (a, b).  Candidate
 *         j's new vertex is m = V_r + j, at (float) (((double) pa + (double) pb) * 0.5) per coordinate.  With T1 = (a, b, c)
 *         the triangle that holds a -> b and T2 = (b, a, d) the one that holds b -> a (each up to rotation): in each of
 *         their rows the corner b becomes m, every other corner stays where it is; the new rows are (m, b, c) for T1 and
 *         (b, m, d) for T2, at T_r + o_j and behind it, T1's first where both exist, o_j the number of triangles of the
 *         candidates before j.  A boundary candidate has only one of the two.
 *      8. Rounds, as step 8 of the flips: the mesh is classified; then, while fewer than maxRounds rounds have run: a round
 *         without a candidate counts, sets converged = 1 and ends the rounds; otherwise it splits every candidate (rounds
 *         counts it, splits and boundarySplits its edges) and the mesh is classified again.  maxRounds = 0 is a pure report.
 *         A mesh in which no triangle takes part has rounds = converged = 1 unless maxRounds = 0.  The limit: a round whose
 *         new rows would take the mesh above maxOutTriangles != 0, or would break outVertices < 2^32 or
 *         3 * outTriangles < 2^32, does not run and is not counted: limited = 1, converged = 0, and the rounds end -- a round
 *         is all or nothing, so the result is that of a call with maxRounds = rounds.  longBefore is the first
 *         classification's number of long edges; longAfter and blockedAfter are the last one's long and blocked edges.  After
 *         convergence longAfter - blockedAfter edges are frozen behind a blocked one.
 *      9. Output.  The V input vertices bit for bit, then the new ones in the order they were made (outVertices); rows
 *         0 .. T - 1 are the input's rows, or what is left of them, in their places, and the new rows follow in the order
 *         they were made (outTriangles).  dOutEnds, if not NULL, gets two uint32 per NEW vertex: the ends a < b of the edge
 *         it halved, in output numbers -- what a caller interpolates normals or colours with.
 *     10. Quality: q of step 9 of the flips, *Before of the input, *After of the output.
 *      What follows: no T-junction is ever made; an input that mlsgpu_hip_mesh_topology calls manifold gives an output with
 *      the same manifold flag, components, boundaries and Euler characteristic, and boundarySplits more boundary edges; after
 *      convergence without pins and irregular edges maxLengthSqAfter <= T; splitting a converged output again returns it bit
 *      for bit; scaling the coordinates and maxLength by a power of two scales the output and changes no count (as long as
 *      nothing leaves the floats' and doubles' normal range). ---- */
typedef struct mlsgpu_split_stats
{
    uint64_t numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t degenerateTriangles;   /* in range, two indices equal */
    uint64_t numEdges;              /* undirected, of the participating triangles */
    uint64_t interiorEdges;         /* step 2 */
    uint64_t boundaryEdges;
    uint64_t rounds, splits, boundarySplits, converged, limited;    /* step 8 */
    uint64_t longBefore, longAfter, blockedAfter;
    uint64_t outVertices, outTriangles;                     /* step 9 */
    double minQualityBefore, minQualityAfter;               /* step 10 */
    double maxLengthSqBefore, maxLengthSqAfter;             /* step 3 */
    uint64_t qualityBefore[16], qualityAfter[16];
} mlsgpu_split_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_split_stats) == 424, "mlsgpu_split_stats is part of the ABI");
#else
typedef char mlsgpu_split_stats_size_is_424[sizeof(mlsgpu_split_stats) == 424 ? 1 : -1];
#endif
/* numVertices packed float xyz and numTriangles uint32 index triples on ctx's device -> dOutVertices / dOutTriangles (and
 * dOutEnds, two uint32 per new vertex, or NULL), with room for capVertices / capTriangles rows (dOutEnds: capVertices -
 * numVertices pairs); no overlap with the inputs, which are left alone.  The capacity rule and the size query are
 * mlsgpu_hip_mesh_repair's: MLSGPU_ERR_LENGTH, with *stats complete and the outputs untouched, if a capacity is below
 * outVertices / outTriangles -- NULL outputs with zero capacities ask for the sizes (and come back MLSGPU_OK if the result is
 * empty).  MLSGPU_ERR_INVALID, before anything touches the device, unless maxLength is finite and > 0, stats is not NULL and
 * maxOutTriangles is 0 or >= numTriangles; MLSGPU_ERR_INVALID for a coordinate that is not finite (counted on the device).
 * MLSGPU_ERR_LENGTH, before anything is allocated, unless numVertices < 2^32 and 3 * numTriangles < 2^32.  No vertices or no
 * triangles is not an error.  Scratch is allocated for the call, grows with the mesh (to at least twice its room whenever a
 * round needs more, by a device-to-device copy, with both copies held while it is made) and is freed on return: per triangle
 * of that room 84 bytes (three side records: the two sides of the sort's 64-bit keys and 32-bit values 72 -- the side the sort
 * leaves free holds the rows a record's split adds and the places of its edge's two sides --, the row's working copy 12), per
 * vertex 12 bytes (the position's working copy) and 8 per new vertex (its ends), the sort's histogram and the scan's tile
 * sums; MLSGPU_ERR_NOMEM if the device does not have it.  Blocks until the statistics are there: one stream synchronisation
 * per classification, to read its counts -- rounds + 1 of them, or rounds where the last round had no candidate or the limit
 * ended them --, one behind each copy of a growing array, one for the sizes and one behind the output. */
int mlsgpu_hip_mesh_split_edges(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                                uint64_t numTriangles, uint32_t maxRounds, double maxLength, uint64_t maxOutTriangles,
                                const uint8_t *dPinned, float *dOutVertices, uint64_t capVertices, uint32_t *dOutTriangles,
                                uint64_t capTriangles, uint32_t *dOutEnds, mlsgpu_split_stats *stats);
/* The same for every output chunk of a finalized device sink, on the mesher's context, by the route of
 * mlsgpu_hip_mesher_fill_holes: every chunk is sized first and then split into new arrays, each chunk behind the one before,
 * and the new generation takes the old one's place only when all chunks are done -- an error leaves the results as they
 * were.  The chunks' normals are dropped.  A chunk's limit is maxGrowth times its triangles; 0 means none.  Chunks are split
 * INDEPENDENTLY.  With more than one chunk a vertex that another chunk has too is pinned, as for the hole filling: an edge of
 * the seam has both ends pinned and is blocked in both chunks, so the seams stay closed bit for bit.  The price is a band of
 * frozen long edges along a seam: they are counted in blockedAfter and longAfter.  *stats: the counts and histograms summed
 * over the chunks, rounds the largest, converged the AND over the chunks that have triangles (without one: as for a mesh
 * without triangles), limited the OR, the two minima the minima and the two maxima the maxima over them.
 * MLSGPU_ERR_INVALID before finalize and unless maxLength is finite and > 0; may be called again. */
int mlsgpu_hip_mesher_split_edges(mlsgpu_mesher *mesher, uint32_t maxRounds, double maxLength, uint32_t maxGrowth,
                                  mlsgpu_split_stats *stats);

/* ---- hole filling of a device-resident mesh: every small boundary loop is capped by a fan of triangles to the mean of its
 *      vertices, before the mesh crosses the link.  An MLS surface stops where the splats get sparse, and
 *      mlsgpu_hip_mesh_topology counts the holes that leaves (numBoundaries); this closes them.  The reference has no
 *      counterpart.  Deterministic: every float and double operation below is ONE correctly rounded IEEE operation (no
 *      contraction), and every sum is an integer sum -- the output depends neither on the schedule nor on the order of the
 *      triangles.
 *      1. A triangle with an index >= V is counted in outOfRangeTriangles (the index is compared, never used as an address);
 *         otherwise a triangle with two equal indices is counted in degenerateTriangles.  Neither takes part; both are
 *         copied to the output unchanged.
 *      2. A participating triangle (a, b, c) gives the directed sides a -> b, b -> c, c -> a.  A directed side a -> b is a
 *         BOUNDARY side if it occurs exactly once and b -> a does not occur at all; boundaryEdges is their number (it agrees
 *         with mlsgpu_smooth_stats.boundaryEdges).
 *      3. A vertex on a boundary side is REGULAR if exactly one boundary side leaves it and exactly one enters it.
 *      4. In the graph whose edges are the boundary sides, a connected component in which every vertex is regular is one
 *         simple directed cycle of n >= 3 sides over n vertices: a LOOP (loops).  The sides of a component with an irregular
 *         vertex are counted in irregularEdges and never filled.  longestLoop is the largest n, 0 without a loop.
 *      5. A loop with n > maxEdges is long (longLoops); otherwise a loop with a pinned vertex is pinned (pinnedLoops); every
 *         other loop is filled (filledLoops): loops = filledLoops + longLoops + pinnedLoops, and filledEdges is the sum of n
 *         over the filled loops.
 *      6. M = the largest |coordinate| over all V input vertices; e is the integer with 2^e <= M < 2^(e + 1) (a subnormal M
 *         has its true exponent), e = 0 if M == 0 or V == 0.  scaleExponent = e, as for the smoothing.
 *      7. Q(x) = llrint(ldexp((double) x, 30 - e)), ties to even.  For a filled loop, per axis, S = the int64 sum of Q over
 *         its n vertices (|S| < 2^51: (double) S is exact); the new vertex is (float) ldexp((double) S / (double) n, e - 30).
 *      8. The filled loops are numbered j = 0, 1, ... in ascending order of their smallest vertex index; loop j's new vertex
 *         has index V + j.
 *      9. Each boundary side a -> b of filled loop j gives the triangle (b, a, V + j): it carries the missing opposite side,
 *         so the orientation is kept.
 *      10. Output vertices: the V input vertices bit for bit, then the new ones.  Output triangles: the T input triangles
 *         bit for bit and in their order, then the new ones -- over all filled loops together -- in ascending order of a
 *         (a regular a leaves exactly one boundary side, so the order is total).
 *      Renumbering the input vertices leaves the output the same as a set of triangles over position triples.  On a
 *      manifold input the output is manifold; per filled loop numBoundaries drops by 1, boundaryEdges by n, and the Euler
 *      characteristic rises by 1.  Scaling every coordinate by 2^s scales the new vertices exactly and moves scaleExponent
 *      by s (away from the subnormals).
 *      Limit: a fan to the mean is meant for small, roughly flat loops.  The outer rim of a small open sheet is a loop like
 *      any other and is capped too: maxEdges is the caller's guard against that. ---- */
#define MLSGPU_FILL_MAX_EDGES 1048576u  /* 2^20 */
typedef struct mlsgpu_fill_stats
{
    uint64_t numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t degenerateTriangles;   /* in range, two indices equal */
    uint64_t boundaryEdges;         /* step 2 */
    uint64_t irregularEdges;        /* boundary sides of components with an irregular vertex */
    uint64_t loops, filledLoops, longLoops, pinnedLoops;        /* steps 4 and 5 */
    uint64_t filledEdges;           /* boundary sides of the filled loops = new triangles */
    uint64_t longestLoop;           /* sides of the longest loop, filled or not */
    uint64_t outVertices;           /* numVertices + filledLoops */
    uint64_t outTriangles;          /* numTriangles + filledEdges */
    int64_t scaleExponent;          /* e of step 6 */
} mlsgpu_fill_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_fill_stats) == 120, "mlsgpu_fill_stats is part of the ABI");
#else
typedef char mlsgpu_fill_stats_size_is_120[sizeof(mlsgpu_fill_stats) == 120 ? 1 : -1];
#endif
/* numVertices packed float xyz and numTriangles uint32 index triples on ctx's device -> dOutVertices with room for
 * capVertices vertices and dOutTriangles with room for capTriangles triangles, which must not overlap the inputs.  dPinned is
 * NULL or one byte per input vertex, non-zero for a pinned one (step 5).  MLSGPU_ERR_INVALID, before anything touches the
 * device, unless 3 <= maxEdges <= MLSGPU_FILL_MAX_EDGES and stats is not NULL; MLSGPU_ERR_LENGTH, before anything is
 * allocated, unless numVertices < 2^32 and 3 * numTriangles < 2^32.  MLSGPU_ERR_INVALID for a coordinate that is not finite
 * (counted on the device).  MLSGPU_ERR_LENGTH if the result would break outVertices < 2^32 or 3 * outTriangles < 2^32.
 * MLSGPU_ERR_LENGTH if capVertices < outVertices or capTriangles < outTriangles: *stats is complete then and the outputs are
 * untouched, which is how a caller asks for the sizes -- NULL outputs with zero capacities.  No vertices or no triangles is
 * not an error.  Scratch is allocated for the call and freed on return: 72 bytes per triangle (three directed side records:
 * the two sides of the sort's 64-bit keys and 32-bit values), 52 bytes per vertex (the boundary forest's parent, the counts
 * of sides out and in, the next vertex, the loop's length, flags and number 4 each, the three sums 24), the sort's histogram
 * and the scan's tile sums; MLSGPU_ERR_NOMEM if the device does not have it.  Blocks until the statistics are there: one stream
 * synchronisation behind the sums (the counts size the result; M stays on the device), and, if the capacities suffice, one
 * at the end. */
int mlsgpu_hip_mesh_fill_holes(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                               uint64_t numTriangles, uint32_t maxEdges, const uint8_t *dPinned, float *dOutVertices,
                               uint64_t capVertices, uint32_t *dOutTriangles, uint64_t capTriangles, mlsgpu_fill_stats *stats);
/* The same for every output chunk of a finalized device sink that has triangles, on the mesher's context.  The chunks GROW:
 * new output arrays of the summed sizes are built, each filled chunk behind the one before, and take the place of the old
 * ones; the chunks' normals are dropped, so normals requested afterwards are those of the filled chunk.  While both
 * generations exist the sink holds 12 bytes per vertex and per triangle of the old AND of the new meshes, plus one chunk's
 * scratch as above and, with more than one chunk, the seam mask: 1 byte per vertex, and 40 bytes per vertex and a sort's
 * histogram while it is built.  Chunks without triangles stay in the list, empty; mlsgpu_hip_mesher_chunk, _chunk_topology,
 * _chunk_normals and _write_ply then serve the filled chunks, and mlsgpu_hip_mesher_stats keeps reporting the finalize's
 * numbers.  *stats is the sum over the chunks, longestLoop and scaleExponent the maxima.
 * SEAMS: the seam between two chunks (split output files) is a boundary of each and must not be capped.  With more than one
 * chunk every vertex whose 12 position bytes equal, as bits, those of a vertex of ANOTHER chunk is pinned -- a welded vertex
 * two chunks share is copied to both with identical bits -- so a loop that touches a seam is counted in pinnedLoops and left
 * open.  A simplify and a smooth under MLSGPU_SMOOTH_BOUNDARY_CURVE move the shared vertices of each chunk on their own and
 * un-match the seams: fill holes BEFORE them.
 * Every chunk runs twice, once for its sizes and once into its place.  MLSGPU_ERR_INVALID before finalize and for a maxEdges
 * outside its range; may be called again (on the filled chunks).  The new arrays take the old ones' place only when every chunk
 * is done: an error leaves the sink's results as they were. */
int mlsgpu_hip_mesher_fill_holes(mlsgpu_mesher *mesher, uint32_t maxEdges, mlsgpu_fill_stats *stats);

/* ---- repair of a device-resident mesh: triangles with a repeated directed side are dropped and pinched vertices are split,
 *      so that a mesh which mlsgpu_hip_mesh_topology calls non-manifold (a simplify can make one) is an oriented manifold
 *      with boundary again before it crosses the link -- what the reference guarantees for everything it writes
 *      (Manifold::isManifold, test/manifold.h:98-232).  Every result is a count, a minimum or a scan: the output depends
 *      neither on the schedule nor, beyond step 6, on the order of the triangles.
 *      1. A triangle with an index >= V is counted in outOfRangeTriangles (the index is compared, never used as an address);
 *         otherwise a triangle with two equal indices is counted in degenerateTriangles -- the rule of the smoothing and the
 *         hole filling, not the topology report's rotation order.  Both kinds are dropped.
 *      2. Every other triangle (a, b, c) gives the directed sides a -> b, b -> c, c -> a.  A directed side that occurs more
 *         than once is REPEATED; repeatedSides counts the occurrences of repeated sides.  Every triangle with a repeated side
 *         is dropped (droppedTriangles) -- all of them, not all but one, so that the result does not depend on the triangles'
 *         order.  An undirected edge of three or more triangles always has a repeated direction, so every edge of the KEPT
 *         triangles has at most two of them, with opposite winding.  Dropping only removes sides: one pass suffices.
 *      3. Among the kept triangles, two corners at one vertex v belong together when one triangle has v -> w and the other
 *         w -> v; the transitive closure gives v's UMBRELLAS.  An umbrella is a RING if every side at v in it has its
 *         opposite among the kept triangles, else a CHAIN.
 *      4. Without flags a vertex is split only where the reference's check fails: where it has at least one ring and more
 *         than one umbrella (MIXED or TUNNEL of the topology report).  Each ring is a GROUP of its own then and all chains
 *         together are one group; every other vertex is one group (the reference allows a vertex on several boundary runs).
 *         Under MLSGPU_REPAIR_SPLIT_PINCHES every umbrella is a group of its own: a topological 2-manifold with boundary,
 *         whose boundary vertices are all regular for the hole filling.
 *      5. A group's key is the smallest `to` over its sides v -> to; the kept sides are unique, so the keys of a vertex
 *         differ.  The output vertices are the groups, numbered densely in ascending (v, key) order; each carries v's 12
 *         position bytes bit for bit.  A vertex that no kept triangle uses disappears (unusedVertices): the reference calls
 *         an isolated vertex non-manifold.  splitVertices counts the input vertices with more than one group, addedVertices
 *         the groups beyond each vertex's first: outVertices = numVertices - unusedVertices + addedVertices.
 *      6. The output triangles are the kept triangles in the input's order, every corner mapped to its group:
 *         outTriangles = numTriangles - outOfRangeTriangles - degenerateTriangles - droppedTriangles.
 *      The topology report of the output has all six counts zero whenever the input has a kept triangle or V = 0 (with
 *      vertices and nothing kept the output is empty).  An input that the report calls manifold comes back bit for bit
 *      without flags.  Permuting the triangles permutes only the output triangles; renumbering the vertices leaves the
 *      output the same as a set of triangles over position triples.  Repairing a repaired mesh changes nothing.
 *      Out of scope: the holes that dropped triangles leave are not re-triangulated (mlsgpu_hip_mesh_fill_holes does). ---- */
#define MLSGPU_REPAIR_SPLIT_PINCHES 1u
typedef struct mlsgpu_repair_stats
{
    uint64_t numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t degenerateTriangles;   /* in range, two indices equal */
    uint64_t repeatedSides;         /* step 2: side records in runs longer than one */
    uint64_t droppedTriangles;      /* step 2: triangles with such a side */
    uint64_t unusedVertices;        /* on no kept triangle */
    uint64_t splitVertices;         /* input vertices with more than one group */
    uint64_t addedVertices;         /* groups beyond the first of their vertex */
    uint64_t outVertices;           /* numVertices - unusedVertices + addedVertices */
    uint64_t outTriangles;          /* numTriangles - outOfRangeTriangles - degenerateTriangles - droppedTriangles */
} mlsgpu_repair_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_repair_stats) == 88, "mlsgpu_repair_stats is part of the ABI");
#else
typedef char mlsgpu_repair_stats_size_is_88[sizeof(mlsgpu_repair_stats) == 88 ? 1 : -1];
#endif
/* numVertices packed float xyz and numTriangles uint32 index triples on ctx's device -> dOutVertices with room for
 * capVertices vertices and dOutTriangles with room for capTriangles triangles, which must not overlap the inputs.  dOutSource
 * is NULL or has room for capVertices uint32: it receives the input index of every output vertex, so that a caller can carry
 * attributes along.  MLSGPU_ERR_INVALID, before anything touches the device, for a NULL ctx or stats and for a flag bit other
 * than MLSGPU_REPAIR_SPLIT_PINCHES; MLSGPU_ERR_LENGTH, before anything is allocated, unless numVertices < 2^32 and
 * 3 * numTriangles < 2^32.  MLSGPU_ERR_LENGTH if capVertices < outVertices or capTriangles < outTriangles: *stats is complete
 * then and the outputs are untouched, which is how a caller asks for the sizes -- NULL outputs with zero capacities (a result
 * that is empty fits them, and the call returns MLSGPU_OK).  Positions are copied, never computed with: a coordinate that is
 * not finite is not an error.  No vertices or no triangles is not an error.  Scratch is allocated for the call and freed on
 * return: 97 bytes per triangle (three directed side records: the two sides of the sort's 64-bit keys and 32-bit values, of
 * which the side the sort leaves free holds the umbrellas' keys, the groups' numbers and the records' flags; the corner
 * forest's parent 12, the chain flags 12, the triangle's state 1), 24 bytes per vertex (its segment's start and end, ring and
 * chain count, smallest chain key, smallest key), the sort's histogram and the scan's tile sums; MLSGPU_ERR_NOMEM if the
 * device does not have it.  Blocks until the statistics are there: one stream synchronisation behind the counts (they size
 * the result), and, if the capacities suffice and the result is not empty, one at the end. */
int mlsgpu_hip_mesh_repair(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                           uint64_t numTriangles, uint32_t flags, float *dOutVertices, uint64_t capVertices,
                           uint32_t *dOutTriangles, uint64_t capTriangles, uint32_t *dOutSource, mlsgpu_repair_stats *stats);
/* The same for every output chunk of a finalized device sink that has triangles, on the mesher's context.  A chunk can GROW
 * in vertices, so the route is that of mlsgpu_hip_mesher_fill_holes: every chunk is sized once and then written once into new
 * output arrays of the summed sizes, each repaired chunk behind the one before, and the new generation takes the old one's
 * place only when every chunk is done -- an error leaves the sink's results as they were.  While both generations exist the
 * sink holds 12 bytes per vertex and per triangle of the old AND of the new meshes, plus one chunk's scratch as above.  The
 * chunks' normals are dropped, so normals requested afterwards are those of the repaired chunk.  Chunks without triangles, and
 * chunks that keep none, stay in the list, empty; mlsgpu_hip_mesher_chunk, _chunk_topology, _chunk_normals and _write_ply
 * then serve the repaired chunks, _simplify, _smooth and _fill_holes work on them, a finalize brings the originals back, and
 * mlsgpu_hip_mesher_stats keeps reporting the finalize's numbers.  *stats is the sum over the chunks.
 * SEAMS: chunks are repaired INDEPENDENTLY, as for simplify and normals.  A vertex two chunks share is split, or not, by
 * each chunk's own triangles; every copy keeps the position bits, so the seam stays closed geometrically and the hole
 * filling's seam matching (equal position bits in another chunk) still sees it.
 * MLSGPU_ERR_INVALID before finalize and for an unknown flag bit; may be called again (on the repaired chunks, which it
 * leaves as they are). */
int mlsgpu_hip_mesher_repair(mlsgpu_mesher *mesher, uint32_t flags, mlsgpu_repair_stats *stats);

/* ---- deviation report of a device-resident mesh: for a set of points (normally the vertices of one mesh) the squared
 *      distance to the surface of another mesh, exact up to a search distance D, with its maximum, a fixed-point mean square,
 *      a histogram and the farthest point.  mlsgpu_hip_mesh_topology says whether a simplified, smoothed or filled mesh is
 *      still a manifold; this says how far it has moved.  The reference has no counterpart.  Deterministic: all arithmetic is
 *      in double on the floats converted exactly, every + - * / below is ONE correctly rounded IEEE operation (no
 *      contraction), dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z, cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z,
 *      u.x*v.y - u.y*v.x), and every field of the report is a count, a minimum, a maximum or an integer sum -- the output
 *      depends neither on the schedule nor on the order of the triangles (but for which of several equal triangles is named).
 *      1. A triangle with an index >= V is counted in outOfRangeTriangles (the index is compared, never used as an address);
 *         otherwise a triangle that names a vertex twice is counted in degenerateTriangles.  Neither takes part.
 *      2. Per axis, lo / hi are the smallest / largest of a triangle's three corner coordinates.  A (point, triangle) pair
 *         is a CANDIDATE iff, on every axis, lo - D <= p and p <= hi + D, each side one double operation.  This belongs to
 *         the contract, not to the implementation: any conservative spatial cull is then exact, since it only has to hand
 *         the kernel a superset of the candidates -- the kernel applies this test before step 3.
 *      3. The squared distance of a candidate pair with corners a, b, c:
 *         seg(p, a, b): u = b - a, w = p - a, L = dot(u, u); s = (L == 0) ? 0 : dot(w, u) / L, then s = fmin(fmax(s, 0), 1);
 *            r = w - s*u (per axis one multiply, one subtract); the value is dot(r, r).
 *         face(p, a, b, c): n = cross(b - a, c - a), nn = dot(n, n); i0 = dot(cross(b - a, p - a), n), i1 = dot(cross(c - b,
 *            p - b), n), i2 = dot(cross(a - c, p - c), n).  If nn > 0 && i0 >= 0 && i1 >= 0 && i2 >= 0, then h = dot(p - a, n)
 *            and the value is (h*h) / nn; otherwise it is +infinity.
 *         d2(p, t) = fmin(fmin(fmin(seg(p,a,b), seg(p,b,c)), seg(p,c,a)), face(p,a,b,c)).
 *         (No data-dependent branch, defined for zero-area triangles and coincident corners, no NaN from finite floats.)
 *      4. D2 = (double) D * (double) D.  best(p) is the smallest d2(p, t) over the point's candidates.  The point is WITHIN if
 *         it has a candidate and best <= D2: its squared distance is best, and its nearest triangle is the LOWEST triangle
 *         index that attains it bit for bit.  Any other point is BEYOND: +infinity, and 0xFFFFFFFF.
 *      5. The report.  farthestPoint: the lowest point index whose squared distance equals maxDistance2, UINT64_MAX if
 *         within == 0.  histogram: a within point goes to the largest k in 0..15 with best >= (D2 * (double)(k*k)) / 256.0
 *         (edges at d = kD/16; best == D2 lands in bin 15).  e = the exponent of D2 (2^e <= D2 < 2^(e + 1)); scaleExponent =
 *         e; q = llrint(best * 2^(30 - e)) <= 2^31; sumQ = the int64 sum of q over the within points (P < 2^32: it fits).
 *         The mean square is sumQ * 2^(e - 30) / within.  maxDistance2: the largest best of a within point, 0 if none.
 *      No points: every field is zero but numVertices, numTriangles, limit2, the triangle counts of step 1 and farthestPoint
 *      (UINT64_MAX).  No triangle that takes part: every point is beyond.  Scaling every coordinate and D by 2^s scales the
 *      distances by 4^s exactly and moves scaleExponent by 2 s (away from overflow and the subnormals). ---- */
typedef struct mlsgpu_deviation
{
    uint64_t numPoints, numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t degenerateTriangles;   /* in range, a vertex twice */
    uint64_t within, beyond;        /* step 4: within + beyond = numPoints */
    uint64_t farthestPoint;         /* step 5 */
    uint64_t farthestChunk;         /* 0; mlsgpu_hip_mesher_deviation: the dense chunk of farthestPoint */
    uint64_t histogram[16];
    int64_t sumQ, scaleExponent;
    double maxDistance2;
    double limit2;                  /* D2 */
} mlsgpu_deviation;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_deviation) == 232, "mlsgpu_deviation is part of the ABI");
#else
typedef char mlsgpu_deviation_size_is_232[sizeof(mlsgpu_deviation) == 232 ? 1 : -1];
#endif
/* numPoints packed float xyz against the mesh of numVertices packed float xyz and numTriangles uint32 index triples, all on
 * ctx's device and none modified.  dDistance2 and dNearest are NULL or hold one entry per point, in the caller's point order
 * (step 4).  MLSGPU_ERR_INVALID, before anything touches the device, for a NULL ctx or out and for a maxDistance that is not
 * finite or is <= 0; MLSGPU_ERR_LENGTH, before anything is allocated, unless numPoints < 2^32, numVertices < 2^32 and
 * 3 * numTriangles < 2^32.  MLSGPU_ERR_INVALID for a point or target coordinate that is not finite (counted on the device).
 * MLSGPU_ERR_LENGTH if the grid's pair count cannot be brought under 2^32.  No points, no vertices or no triangles is not an
 * error.  The cull is a sparse uniform grid over the target's box: a triangle is paired with every cell that its box, inflated
 * by D, touches, and a point is tested against the pairs of its own cell; the cell size is doubled until the pairs number at
 * most max(2^20, 8 per triangle).  Scratch is allocated for the call and freed on return: 24 bytes per point (the two sides of
 * a sort's 64-bit keys and 32-bit values) and 8 more where dDistance2 is NULL, 8 bytes per triangle (its cell count and where
 * its pairs begin), 24 bytes per grid pair, the sorts' histograms and the scan's tile sums; MLSGPU_ERR_NOMEM if the device
 * does not have it.  Blocks until the report is there. */
int mlsgpu_hip_mesh_deviation(mlsgpu_ctx *ctx, const float *dPoints, uint64_t numPoints, const float *dVertices,
                              uint64_t numVertices, const uint32_t *dTriangles, uint64_t numTriangles, float maxDistance,
                              double *dDistance2, uint32_t *dNearest, mlsgpu_deviation *out);
/* The reference that mlsgpu_hip_mesher_deviation measures against: on a finalized device sink, copies every chunk's current
 * vertices and triangles, and the chunk spans, into device arrays that the mesher holds (12 bytes per vertex and per
 * triangle).  Call it directly behind finalize, before a stage that moves vertices.  MLSGPU_ERR_INVALID before finalize;
 * calling it again replaces the copy.  mlsgpu_hip_mesher_reset and _destroy free it; a new finalize keeps it only if the chunk
 * list has the same length, and drops it otherwise.  _drop_reference frees it (no reference is not an error). */
int mlsgpu_hip_mesher_keep_reference(mlsgpu_mesher *mesher);
int mlsgpu_hip_mesher_drop_reference(mlsgpu_mesher *mesher);
/* The deviation of a finalized device sink from its kept reference, chunk by chunk over the dense chunk list (which the stages
 * keep stable: a chunk that lost its triangles stays in it).  *moved: the current chunk's vertices against the kept chunk's
 * surface -- how far the output left the original.  *lost: the kept chunk's vertices against the current chunk's surface --
 * what the original had that the output flattened.  Either may be NULL.  Over the chunks the counts, the histogram and sumQ
 * add (D is the same, hence the scale); maxDistance2 is the maximum, and farthestChunk / farthestPoint name the lowest (dense
 * chunk index, point index within the chunk) that attains it.  MLSGPU_ERR_INVALID before finalize, without a kept reference
 * and for a refused maxDistance.  Changes nothing in the sink; works after any sequence of fill / simplify / repair / smooth. */
int mlsgpu_hip_mesher_deviation(mlsgpu_mesher *mesher, float maxDistance, mlsgpu_deviation *moved, mlsgpu_deviation *lost);

/* ---- self-intersection report of a device-resident mesh: the pairs of triangles that CERTAINLY pass through each other.
 *      mlsgpu_hip_mesh_topology says whether a simplified, smoothed or filled mesh is still a manifold and
 *      mlsgpu_hip_mesh_deviation how far it moved; a surface that a stage pulled through itself is a perfect manifold with a
 *      small deviation, and this report is what sees it.  The reference has no counterpart.  Deterministic: all arithmetic is
 *      in double on the floats converted exactly, every + - * below is ONE correctly rounded IEEE operation (no contraction),
 *      dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z, cross(u, v) = (u.y*v.z - u.z*v.y, u.z*v.x - u.x*v.z, u.x*v.y - u.y*v.x),
 *      and every field of the report is a count, a minimum or a maximum -- the output does not depend on the schedule, and the
 *      order of the triangles changes only which indices are named.
 *      1. A triangle with an index >= V is counted in outOfRangeTriangles (the index is compared, never used as an address);
 *         otherwise a triangle that names a vertex twice is counted in degenerateTriangles.  Neither takes part.
 *      2. Per axis, lo / hi are the smallest / largest of a triangle's three corner coordinates.  Two triangles A < B (by
 *         index) that take part are a CANDIDATE pair iff, on every axis, loA <= hiB and loB <= hiA, as float comparisons.
 *         This belongs to the contract, not to the implementation: any conservative spatial cull is then exact.
 *         candidatePairs counts them, neighbours included.
 *      3. The certain sign orient(a, b, c, x): r0 = a - x, r1 = b - x, r2 = c - x; det = dot(r0, cross(r1, r2)); perm is the
 *         same expression with the six products of the cross and the three of the dot taken over absolute values -- with
 *         p = (|r1.y*r2.z| + |r1.z*r2.y|, |r1.z*r2.x| + |r1.x*r2.z|, |r1.x*r2.y| + |r1.y*r2.x|), perm = (|r0.x|*p.x +
 *         |r0.y|*p.y) + |r0.z|*p.z, a sum of non-negative terms in the same order.  The sign is 0 if |det| <= perm * 2^-48,
 *         otherwise the sign of det.  The constant is derived, not tuned: the forward error of this evaluation on exact
 *         differences is below 8 * 2^-53 * perm (Shewchuk's static filter for orient3d), the three rounded differences add
 *         less than 2^-50 * perm; so, away from underflow, a sign that is not 0 is the true sign.  An x equal in coordinates
 *         to a, b or c gives a zero row or a zero cross product, hence det == perm * 0 == 0 exactly: shared corners need no
 *         index test, and welded duplicates behave like shared ones.
 *      4. Side (p, q) PIERCES triangle (a, b, c) iff orient(a,b,c,p) * orient(a,b,c,q) < 0 and s0 = orient(p,q,a,b), s1 =
 *         orient(p,q,b,c), s2 = orient(p,q,c,a) are all nonzero and equal.  (Every sign is a function of its twelve
 *         coordinates alone: whether an implementation works out one it does not need cannot change a result.)
 *      5. A candidate pair CROSSES iff one of A's sides (a, b), (b, c), (c, a) pierces B or one of B's pierces A, in the
 *         stored corner order.
 *      6. The report.  crossingPairs; crossingTriangles: the triangles with at least one partner; lowestA, lowestB: the
 *         lexicographically lowest crossing pair, UINT64_MAX each if there is none; maxPartners: the most partners of one
 *         triangle, and maxPartnersTriangle the lowest index that attains it, UINT64_MAX if there is no crossing.
 *      THE LIMIT: the report says "these pairs certainly pass through each other" and is a lower bound.  Touching, coplanar
 *      overlap and whatever rests on an uncertain sign are deliberately not reported; two neighbours folded flat onto each
 *      other are not found (a smoothing fold shows through the next ring of triangles). ---- */
typedef struct mlsgpu_self_intersections
{
    uint64_t numVertices, numTriangles;
    uint64_t outOfRangeTriangles;   /* an index >= numVertices */
    uint64_t degenerateTriangles;   /* in range, a vertex twice */
    uint64_t candidatePairs;        /* step 2 */
    uint64_t crossingPairs;         /* step 5 */
    uint64_t crossingTriangles;
    uint64_t lowestA, lowestB;
    uint64_t maxPartners, maxPartnersTriangle;
    uint64_t lowestChunk;           /* 0; mlsgpu_hip_mesher_self_intersections: the dense chunk of lowestA / lowestB */
    uint64_t crossingChunks;        /* 0; mlsgpu_hip_mesher_self_intersections: the chunks with a crossing pair */
} mlsgpu_self_intersections;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_self_intersections) == 104, "mlsgpu_self_intersections is part of the ABI");
#else
typedef char mlsgpu_self_intersections_size_is_104[sizeof(mlsgpu_self_intersections) == 104 ? 1 : -1];
#endif
/* The mesh of numVertices packed float xyz and numTriangles uint32 index triples on ctx's device, not modified.  dPartners is
 * NULL or holds one uint32 per triangle: the number of its partners, 0 for a triangle that takes no part.  dPairs is NULL or
 * has room for pairCapacity rows of two uint32 (A, B), A < B: the crossing pairs in ascending lexicographic order.  The
 * capacity rule is mlsgpu_hip_mesh_fill_holes': with a dPairs and pairCapacity < crossingPairs the call returns
 * MLSGPU_ERR_LENGTH, *out (and dPartners) complete and the list untouched, which is how a caller asks for the size; a NULL
 * dPairs asks for no list and is no error.  MLSGPU_ERR_INVALID, before anything touches the device, for a NULL ctx or out;
 * MLSGPU_ERR_LENGTH, before anything is allocated, unless numVertices < 2^32 and 3 * numTriangles < 2^32.
 * MLSGPU_ERR_INVALID for a coordinate that is not finite (counted on the device).  MLSGPU_ERR_LENGTH if the grid's record
 * count cannot be brought under 2^32, or for 2^32 crossing pairs or more where the list is taken.  No vertices or no triangles
 * is not an error.  The cull is a sparse uniform grid over the mesh's box: a triangle has a record in every cell its box
 * touches, and a pair is looked at in the one cell that holds the larger of the two boxes' lower corners per axis; the cell
 * size starts at the mean extent of a triangle's box and is doubled until the records number at most max(2^20, 8 per
 * triangle).  Scratch is allocated for the call and freed on return: 16 bytes per triangle (its cell count, where its records
 * begin, the cell of its lower corner) and 4 more where dPartners is NULL, 24 bytes per grid record (the two sides of a
 * sort's 64-bit keys and 32-bit values), 24 bytes per crossing pair where the list is written, the sorts' histograms and the
 * scan's tile sums; MLSGPU_ERR_NOMEM if the device does not have it.  Blocks until the report is there. */
int mlsgpu_hip_mesh_self_intersections(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices,
                                       const uint32_t *dTriangles, uint64_t numTriangles, uint32_t *dPartners,
                                       uint32_t *dPairs, uint64_t pairCapacity, mlsgpu_self_intersections *out);
/* The same for a finalized device sink, chunk by chunk over the dense chunk list.  The counts add; maxPartners is the maximum
 * and maxPartnersTriangle the triangle, within the lowest chunk that attains it, that the chunk's report names;
 * lowestChunk / lowestA / lowestB name the lowest (dense chunk index, A, B) and crossingChunks counts the chunks that have a
 * crossing pair.  THE LIMIT: crossings between triangles of different chunks are not looked for.  MLSGPU_ERR_INVALID before
 * finalize.  Changes nothing in the sink; works after any sequence of fill / simplify / repair / smooth. */
int mlsgpu_hip_mesher_self_intersections(mlsgpu_mesher *mesher, mlsgpu_self_intersections *out);

/* ---- compact read-back of a device-resident mesh: the SAME mesh in fewer bytes for the link to the host.  A chunk leaves HBM
 *      as 12 bytes per vertex and 12 per triangle; the sink numbers vertices block by block and slice by slice, so the indices of
 *      64 consecutive triangles lie within a few thousand of each other, and a frame-of-reference code per 64 triangles with an
 *      exception list holds them in about a third.  Triangles are lossless; vertices are bit-exact at vertexBits = 32 and
 *      quantised to a stated bound below.  The reference has no counterpart.  THE FORMAT, version 1: a blob is a sequence of
 *      little-endian 32-bit words; its bytes are a function of the input arrays and vertexBits only (every field is a minimum, a
 *      count, a scan or an OR of disjoint bits), and all padding bits are zero.  A BIT STREAM of values of b bits: value i
 *      occupies bits [i*b, (i+1)*b), bit j of the stream is bit (j mod 32) of word j / 32, the stream ends with the word that
 *      holds its last bit.
 *      1. Header, 16 words: 0 magic "MLSC" (0x43534C4D); 1 version 1; 2 vertexBits; 3 group size 64; 4-5 numVertices (low word
 *         first); 6-7 numTriangles; 8-10 lo and 11-13 hi as float bits per axis; 14-15 the words of the whole blob.
 *      2. Vertex section.  vertexBits b is 32 or lies in 8..24.  b = 32: the 3 V floats copied as bits (any bit pattern), lo = hi
 *         = 0.  b < 32: lo / hi per axis are the minimum / maximum as INTEGERS after the order-preserving map of float bits to
 *         uint32 (u = bits ^ 0xFFFFFFFF for a set sign bit, bits | 0x80000000 otherwise: a total order with -0 < +0), both +0 for
 *         no vertices.  d = double(hi) - double(lo); q = 0 if d = 0, otherwise q = floor((double(x) - double(lo)) *
 *         (double(2^b - 1) / d) + 0.5) clamped to [0, 2^b - 1], every operation ONE correctly rounded double operation (no
 *         contraction).  The section is the bit stream of the 3 V values q of b bits, vertex v axis a being value 3 v + a.
 *         Decoding: x' = float(double(lo) + double(q) * (d / double(2^b - 1))), and |x' - x| <= 0.5 * d / (2^b - 1) +
 *         ulp32(max(|lo|, |hi|)) per axis.
 *      3. Triangle section.  G = ceil(T / 64) groups of n <= 64 consecutive triangles.  G + 1 offsets, in words relative to the
 *         first group record, the first 0 and the last the length of all records; then the records.  A group has 3 n SLOTS, slot
 *         3 t + k being corner k of its triangle t; base is its smallest index and a slot's value v = index - base.  For a width
 *         w in 1..31, v is INLINE if v < 2^w - 1; otherwise the slot holds the escape 2^w - 1 and v joins the group's exception
 *         list, in slot order.  w = 32 has no exceptions.  cost(w) = 4 * ceil(3 n w / 32) + 4 * exceptions(w), and the group
 *         takes the smallest w of minimum cost.  A record: base; the word w | exceptions << 8; the bit stream of the 3 n slot
 *         values of w bits; the exceptions.  Indices are not compared with numVertices: any uint32 triples come back bit for bit
 *         and in their order.
 *      Normals are not part of the format. ---- */
#define MLSGPU_COMPACT_MAGIC 0x43534C4Du
#define MLSGPU_COMPACT_VERSION 1u
#define MLSGPU_COMPACT_GROUP 64u
#define MLSGPU_COMPACT_HEADER_WORDS 16u
typedef struct mlsgpu_compact_stats
{
    uint64_t numVertices, numTriangles;
    uint64_t vertexBits;
    uint64_t blobBytes;             /* 64 + vertexBytes + triangleBytes */
    uint64_t vertexBytes;           /* the vertex section */
    uint64_t triangleBytes;         /* offsets and records */
    uint64_t groups;
    uint64_t exceptions;            /* over all groups */
    uint64_t widthHistogram[33];    /* [w]: the groups of width w; [0] stays 0 */
    double step[3];                 /* d / (2^b - 1) per axis: a decoded coordinate is lo + q * step; 0 for b = 32 or d = 0 */
} mlsgpu_compact_stats;
#ifdef __cplusplus
static_assert(sizeof(mlsgpu_compact_stats) == 352, "mlsgpu_compact_stats is part of the ABI");
#else
typedef char mlsgpu_compact_stats_size_is_352[sizeof(mlsgpu_compact_stats) == 352 ? 1 : -1];
#endif
/* Encodes the mesh of numVertices packed float xyz and numTriangles uint32 index triples on ctx's device, not modified, into
 * the capacityBytes at dOut (device memory, 4-byte aligned, not overlapping the inputs).  The capacity rule is
 * mlsgpu_hip_mesh_fill_holes': with a dOut that is NULL or holds fewer than blobBytes, the planning pass alone runs, *stats is
 * complete, the output is untouched and the call returns MLSGPU_ERR_LENGTH, which is how a caller asks for the size; bytes of
 * dOut beyond blobBytes are never written.  MLSGPU_ERR_INVALID, before anything touches the device, for a NULL ctx or stats, a
 * vertexBits that is not 32 or in 8..24, a dOut that is not 4-byte aligned; MLSGPU_ERR_LENGTH, before anything is allocated,
 * unless numVertices < 2^32, 3 * numTriangles < 2^32 and 194 words for every group stay below 2^32 (the longest record a group
 * can have: a record stream of 2^32 words or more cannot be addressed by its offsets).  MLSGPU_ERR_INVALID for vertexBits < 32
 * and a coordinate that is not finite (counted on the device); at 32 any bits pass.  No vertices or no triangles is not an
 * error.  Three kernels plan: the extents (integer min / max), one wave per group (base by a wave minimum, the exceptions of
 * every width from the bit lengths of the 192 values, the arg-min cost) and a scan of the record lengths; three write: header,
 * vertices and groups, each bit stream assembled in a tile of on-chip memory and stored as whole words.  Scratch is allocated
 * for the call and freed on return: 12 bytes per group (base, width and exceptions, offset), the scan's tile sums (4 bytes per
 * 2048 groups) and 312 bytes of counters; MLSGPU_ERR_NOMEM if the device does not have it.  Blocks until the blob is there. */
int mlsgpu_hip_mesh_compact(mlsgpu_ctx *ctx, const float *dVertices, uint64_t numVertices, const uint32_t *dTriangles,
                            uint64_t numTriangles, uint32_t vertexBits, void *dOut, uint64_t capacityBytes,
                            mlsgpu_compact_stats *stats);
/* Output chunk i of a finalized device sink (after any fill / simplify / repair / smooth), encoded into device scratch of
 * blobBytes and copied into the caller's HOST memory, pinned or not.  The same capacity rule: a NULL hostBlob or too few
 * capacityBytes return MLSGPU_ERR_LENGTH with *stats complete and nothing written or allocated for the blob.
 * MLSGPU_ERR_INVALID before finalize or for an i that is no output chunk.  Leaves the sink's arrays and cached normals
 * untouched. */
int mlsgpu_hip_mesher_chunk_compact(mlsgpu_mesher *mesher, uint32_t i, uint32_t vertexBits, void *hostBlob, uint64_t capacityBytes,
                                    mlsgpu_compact_stats *stats);
/* The host side: no GPU and no HIP call.  The blob is UNTRUSTED: both calls validate every header field, every offset and every
 * record of the `bytes` at `blob` (4-byte aligned) before anything is written, and return MLSGPU_ERR_FORMAT unless: bytes is
 * exactly the header's word count times 4; magic, version and group size are the format's; vertexBits is 32 or in 8..24;
 * numVertices < 2^32 and 3 * numTriangles < 2^32; lo = hi = 0 as bits at 32, both finite with lo <= hi in the integer order
 * below; the sections fill the blob exactly; the offsets start at 0, rise by exactly each record's length and end at the
 * records' length; every w is in 1..32; exceptions <= slots, and the escapes among the slots number the exceptions (none at
 * w = 32); base + v does not wrap.  Nothing outside the given buffers is read or written.  MLSGPU_ERR_INVALID for a NULL or
 * misaligned blob or a NULL stats / output that is needed.  _info fills *stats from the blob (step as the decoder uses it).
 * _decode writes numVertices packed xyz to `vertices` and numTriangles triples to `triangles` (the caller sizes them from
 * _info); groups and vertex ranges are spread over `threads` std::threads, 0 meaning 8, at most 64, for the validation as
 * for the writing. */
int mlsgpu_hip_compact_info(const void *blob, uint64_t bytes, mlsgpu_compact_stats *stats);
int mlsgpu_hip_compact_decode(const void *blob, uint64_t bytes, float *vertices, uint32_t *triangles, uint32_t threads);

/* ---- host mesh sink: OOCMesher's weld as the reference runs it, on the host (src/mesher.cpp:220-469, north_star:
 *      "welding stays on host").  add() is MesherBase::InputFunctor: local components of the block by union-find over
 *      two edges per triangle (computeLocalComponents, :220-236), clumps merged across blocks through the external
 *      keys (updateClumpKeyMap, :286-311); finalize() applies the prune rule of getStatistics (:491-536) and lays out
 *      one mesh per chunk in which a key appears once (externalRemap, :538-567).  Meshes of ANY device can be added --
 *      it is the cross-GPU welder behind mlsgpu_hip_farm_set_host_output.  In memory: no temporary files, no reorder
 *      buffer; chunk ids may arrive interleaved.  add() is serialised by an internal mutex. ---- */
typedef struct mlsgpu_host_mesher mlsgpu_host_mesher;
int mlsgpu_hip_host_mesher_create(mlsgpu_host_mesher **out);
/* The welders' memory is mapped in slabs that the PROCESS keeps when a welder is destroyed (up to 16 GiB, or
 * MLSGPU_HIP_WELDER_CACHE_MB), because freshly mapped memory faults in slowly; the memory a welder gets is uninitialised.
 * _trim_cache sets that limit and returns what is held beyond it to the system at once (0: keep nothing); it returns the
 * bytes released.  The reference's mesher allocates per job (src/mesher.cpp:220-306) and has no counterpart. */
uint64_t mlsgpu_hip_host_mesher_trim_cache(uint64_t keepBytes);
void mlsgpu_hip_host_mesher_destroy(mlsgpu_host_mesher *mesher);
int mlsgpu_hip_host_mesher_set_prune_threshold(mlsgpu_host_mesher *mesher, double threshold);
/* Threads of the welder: add() copies the block and queues its work (local components, key map: OOCMesher::add,
 * src/mesher.cpp:370-469) as a task, and finalize builds the output block by block on the same pool (the reference runs
 * one mesher thread and parallelises its heavy rewrite with OpenMP, src/mesher.cpp:597-600).  0 = default:
 * MLSGPU_HIP_HOST_MESHER_THREADS, else min(32, hardware threads).  Before the first add; results do not depend on it. */
int mlsgpu_hip_host_mesher_set_threads(mlsgpu_host_mesher *mesher, uint32_t threads);
uint32_t mlsgpu_hip_host_mesher_threads(mlsgpu_host_mesher *mesher);
/* The welder's threads bound to the CPUs of ONE NUMA node -- the node its meshes arrive on (mlsgpu_hip_farm_placement
 * out[1]: the read-back ring is next to the farm's first GPU), so that a block's pieces are welded within one socket's
 * caches.  -1 (default): unbound.  Before the first add.  The reference's mesher thread is not placed. */
int mlsgpu_hip_host_mesher_set_node(mlsgpu_host_mesher *mesher, int node);
int mlsgpu_hip_host_mesher_node(mlsgpu_host_mesher *mesher);
/* Bounded-memory mode -- OOCMesher's temporary files (src/mesher.cpp:404-419 writes every block's vertices and triangles to
 * them, :763-852 reads them back): the welder's memory becomes mappings of nameless temporary files in `dir`, and once more
 * than `residentBytes` of blocks have arrived a block is written out and dropped from memory when its task is done; the
 * output passes fault it back in.  Results are the in-memory mode's, element for element.  Before the first add; an unusable
 * directory is MLSGPU_ERR_INVALID; NULL or "" = in memory (the default).  tmp_usage: out[0] = bytes of temporary files mapped,
 * out[1] = of which in memory right now, out[2] = bytes of blocks handed to the kernel to write out and drop. */
int mlsgpu_hip_host_mesher_set_tmp_dir(mlsgpu_host_mesher *mesher, const char *dir, uint64_t residentBytes);
int mlsgpu_hip_host_mesher_tmp_usage(mlsgpu_host_mesher *mesher, uint64_t out[3]);
int mlsgpu_hip_host_mesher_add(mlsgpu_host_mesher *mesher, uint64_t chunkId, const mlsgpu_host_mesh *mesh);
/* a mlsgpu_farm_host_output_fn whose `user` is the mlsgpu_host_mesher */
int mlsgpu_hip_host_mesher_farm_output(void *mesher, int device, uint64_t chunkId, const mlsgpu_host_mesh *mesh);
/* Ship-outs that arrive IN PLACE.  landing: `bytes` of the welder's own memory (page-locked where the process has a GPU:
 * landing_pinned says so), valid until the welder is destroyed; add_landed: add() for a mesh whose arrays lie in such
 * memory -- adopted, not copied (the index check that rides on add()'s copy runs first thing in the block's task: a bad mesh
 * makes finalize fail with MLSGPU_ERR_INVALID).  farm_landing / farm_output_landed: the pair for
 * mlsgpu_hip_farm_set_host_landing, `user` = the mesher. */
int mlsgpu_hip_host_mesher_landing(mlsgpu_host_mesher *mesher, uint64_t bytes, void **out);
int mlsgpu_hip_host_mesher_landing_pinned(mlsgpu_host_mesher *mesher);
int mlsgpu_hip_host_mesher_add_landed(mlsgpu_host_mesher *mesher, uint64_t chunkId, const mlsgpu_host_mesh *mesh);
int mlsgpu_hip_host_mesher_farm_landing(void *mesher, uint64_t bytes, void **out);
int mlsgpu_hip_host_mesher_farm_output_landed(void *mesher, int device, uint64_t chunkId, const mlsgpu_host_mesh *mesh);
int mlsgpu_hip_host_mesher_finalize(mlsgpu_host_mesher *mesher, uint32_t *numChunks);
/* Output chunk i (chunks in order of first arrival, those without triangles skipped): host pointers, valid until the
 * next add / finalize / destroy; indices relative to the chunk's first vertex. */
int mlsgpu_hip_host_mesher_chunk(mlsgpu_host_mesher *mesher, uint32_t i, uint64_t *chunkId, uint64_t *numVertices,
                                 uint64_t *numTriangles, const float **vertices, const uint32_t **triangles);
/* as mlsgpu_hip_mesher_stats */
int mlsgpu_hip_host_mesher_stats(mlsgpu_host_mesher *mesher, uint64_t out[8]);
/* Several meshers, one job (one process per GPU, each welding its own buckets; the reference's MPI build gathers every
 * ship-out on one rank instead, src/mlsgpu_mpi.cpp).  Components that cross rank boundaries and the prune threshold need
 * the other ranks' clumps: boundary() sizes and boundary_read() exports every external key this mesher has seen (sorted)
 * with the ROOT clump holding its vertex, and the vertex / triangle counts of every root clump (0 for the others).  The
 * caller unites clumps that share a key across meshers (a vertex seen by r meshers was counted r times), applies the
 * prune rule of getStatistics (src/mesher.cpp:491-536) to the merged counts and hands the verdict per root clump back
 * to finalize_with().  mlsgpu_amd/dist_sink.py does this over torch.distributed. */
int mlsgpu_hip_host_mesher_boundary(mlsgpu_host_mesher *mesher, uint64_t *numKeys, uint64_t *numClumps);
int mlsgpu_hip_host_mesher_boundary_read(mlsgpu_host_mesher *mesher, uint64_t *keys, uint32_t *keyClump,
                                         uint64_t *clumpVertices, uint64_t *clumpTriangles);
int mlsgpu_hip_host_mesher_finalize_with(mlsgpu_host_mesher *mesher, const uint8_t *keepClump, uint64_t numClumps,
                                         uint32_t *numChunks);

/* Output chunk i of a finalized mesher (mlsgpu_hip_mesher_chunk) written as FastPly::Writer's file STRAIGHT FROM HBM through
 * two pinned buffers of bufferBytes / 2 (0 = 64 MiB): while one piece is written the next travels, faces are packed into the
 * file's 13-byte records on the device, and the host never holds more of the mesh than the buffer -- the role of the
 * reference's asynchronous writer (src/async_io.h:95-140) for outputs larger than host memory.  Same bytes as
 * mlsgpu_hip_write_ply of the downloaded arrays. */
int mlsgpu_hip_mesher_write_ply(mlsgpu_mesher *mesher, uint32_t i, const char *path, const char *const *comments,
                                uint32_t numComments, uint64_t bufferBytes);

/* FastPly::Writer's file from host memory (src/fast_ply.cpp:443-521): binary little endian, header padded to 4 bytes,
 * float32 x y z, faces as uint8 3 + 3 x uint32 */
int mlsgpu_hip_write_ply(const char *path, const float *vertices, uint64_t numVertices, const uint32_t *triangles,
                         uint64_t numTriangles, const char *const *comments, uint32_t numComments);

/* The same files with the vertex normals: property float32 nx / ny / nz after z, 24-byte vertex rows, everything else as
 * above.  Host memory in (normals: 3 floats per vertex) ... */
int mlsgpu_hip_write_ply_normals(const char *path, const float *vertices, const float *normals, uint64_t numVertices,
                                 const uint32_t *triangles, uint64_t numTriangles, const char *const *comments,
                                 uint32_t numComments);
/* ... or output chunk i of a finalized mesher straight from HBM through the two pinned buffers of
 * mlsgpu_hip_mesher_write_ply, the rows interleaved on the device as the faces are packed: the chunk's normals are those of
 * mlsgpu_hip_mesher_chunk_normals, computed now if nobody asked for them yet.  Same bytes as mlsgpu_hip_write_ply_normals of
 * the downloaded arrays. */
int mlsgpu_hip_mesher_write_ply_normals(mlsgpu_mesher *mesher, uint32_t i, const char *path, const char *const *comments,
                                        uint32_t numComments, uint64_t bufferBytes);

/* ---- splat input: FastPly::Reader, src/fast_ply.h:77-262; host only ---- */
typedef struct mlsgpu_ply_reader mlsgpu_ply_reader;
/* Opens a binary PLY file of splats (float32 x y z nx ny nz radius among the vertex properties) and checks its header;
 * MLSGPU_ERR_FORMAT with the reference's message otherwise.  radius' = min(radius, maxRadius) * smooth,
 * quality = 1 / radius'^2 (Reader::decode, src/fast_ply.cpp:334-350). */
int mlsgpu_hip_ply_open(const char *path, float smooth, float maxRadius, mlsgpu_ply_reader **out);
void mlsgpu_hip_ply_close(mlsgpu_ply_reader *reader);
uint64_t mlsgpu_hip_ply_size(const mlsgpu_ply_reader *reader);
/* out[0] vertex size in bytes, [1] vertex count, [2] header size, [3..9] byte offsets of x y z nx ny nz radius */
int mlsgpu_hip_ply_layout(const mlsgpu_ply_reader *reader, uint64_t out[10]);
/* Reader::Handle::read: splats [first, first + count) into host memory (e.g. what mlsgpu_hip_farm_acquire returned) */
int mlsgpu_hip_ply_read(mlsgpu_ply_reader *reader, uint64_t first, uint64_t count, mlsgpu_splat *out);
/* File -> device memory, decode (hostThreads host threads, 0 = 4) overlapped with the host-to-device copies through two
 * pinned 64 MiB buffers on ctx's stream; returns when dOut[0 .. count) is complete.  What the reference's reader
 * threads + async I/O do for its out-of-core splat sets (src/splat_set.h:389-700), for inputs that fit in HBM. */
int mlsgpu_hip_ply_load(mlsgpu_ply_reader *reader, mlsgpu_ctx *ctx, uint64_t first, uint64_t count, mlsgpu_splat *dOut,
                        uint32_t hostThreads);

/* ---- SplatSet::FileSet, src/splat_set.h:383-700: several PLY files read as ONE splat sequence
 *      (file after file; the reference packs the file number into the upper bits of its splat ids, here ids are
 *      positions in the concatenation). ---- */
typedef struct mlsgpu_fileset mlsgpu_fileset;
int mlsgpu_hip_fileset_create(float smooth, float maxRadius, mlsgpu_fileset **out);
void mlsgpu_hip_fileset_destroy(mlsgpu_fileset *files);
/* FileSet::addFile: the header is parsed and checked now (MLSGPU_ERR_FORMAT as mlsgpu_hip_ply_open) */
int mlsgpu_hip_fileset_add_file(mlsgpu_fileset *files, const char *path);
uint64_t mlsgpu_hip_fileset_num_files(const mlsgpu_fileset *files);
uint64_t mlsgpu_hip_fileset_num_splats(const mlsgpu_fileset *files);     /* FileSet::maxSplats */
/* FileSet::setBufferSize (default 32 MiB): the host memory a load may hold, whatever the size of the files */
int mlsgpu_hip_fileset_set_buffer_size(mlsgpu_fileset *files, uint64_t bytes);
/* splats [first, first + count) of the sequence into host memory (e.g. what mlsgpu_hip_farm_acquire returned) */
int mlsgpu_hip_fileset_read(mlsgpu_fileset *files, uint64_t first, uint64_t count, mlsgpu_splat *out);
/* The same range into DEVICE memory with bounded host memory: `readerThreads` host threads (0 = 4; the reference's
 * ReaderThread, src/splat_set.h:560-700) fill the slots of one pinned buffer of the set's buffer size with consecutive
 * chunks while earlier chunks travel to the GPU on ctx's stream (the role of src/async_io.h:95-140 + CopyGroup for
 * clouds that fit in HBM: 10^9 splats are 32 GB of 288).  When every file's rows are whole 32-bit words no wider than a
 * splat (x y z nx ny nz radius as float32: 28 bytes) the threads only READ the rows, the rows cross the link as the file
 * holds them and a kernel decodes them (Reader::decode, src/fast_ply.cpp:374-400: same splats bit for bit); any other
 * layout, or MLSGPU_HIP_FILESET_RAW=0, is decoded by the threads.  8-16 threads on the GPU's NUMA node reach the link's
 * rate (61 GB/s of splats); the staging is kept by the set from call to call.  One load per set at a time.  Returns when
 * dOut[0 .. count) is complete. */
int mlsgpu_hip_fileset_load(mlsgpu_fileset *files, mlsgpu_ctx *ctx, uint64_t first, uint64_t count, mlsgpu_splat *dOut,
                            uint32_t readerThreads);
/* Bucket::bucket over a FileSet that need NOT fit the device -- the role of the reference's blob index and host bucketing
 * (FastBlobSet, src/splat_set.h:713-905; bucketRecurse, src/bucket_impl.h:439-560) for data beyond HBM.  The files are
 * streamed through a chunk buffer of `chunkSplats` splats: once to count the level's microblock octree (the reference's first
 * pass over the blobs), then once per BATCH of top-level regions that fit `budgetSplats` splats together (its second); a
 * batch is resident while its regions are split further and its buckets handed to `fn`, whose mlsgpu_bucket::dSplats is the
 * batch and dIds positions in it (valid during the callback: mlsgpu_hip_farm_submit_device copies the bucket out).  The
 * buckets -- extents, order, member splats in file order -- are those mlsgpu_hip_bucket makes of the same set resident.
 * stats (may be NULL): [0] passes over the files, [1] batches, [2] splats loaded into batches, [3] file chunks a pass did
 * not have to read (the first pass notes every chunk's bounding box; a batch skips the chunks that stay clear of its regions).
 * MLSGPU_ERR_LENGTH if one top-level region alone exceeds the budget. */
/* FastBlobSet::makeBoundingGrid (src/splat_set_impl.h:770-811) for such a set: one pass over the files through a chunk buffer.
 * MLSGPU_ERR_LENGTH, *out not written, if an extent does not fit int32 (as mlsgpu_hip_bounding_grid). */
int mlsgpu_hip_fileset_bounding_grid(mlsgpu_fileset *files, mlsgpu_ctx *ctx, float spacing, uint32_t bucketSize,
                                     uint64_t chunkSplats, uint32_t readerThreads, mlsgpu_grid *out);
int mlsgpu_hip_bucket_stream(mlsgpu_ctx *ctx, mlsgpu_fileset *files, const mlsgpu_grid *region,
                             const mlsgpu_bucket_params *params, uint64_t budgetSplats, uint64_t chunkSplats,
                             uint32_t readerThreads, mlsgpu_bucket_fn fn, void *user, uint64_t *cellSplats, uint64_t stats[4]);

/* DeviceWorkerGroupBase::computeMaxSwathe, src/workers.cpp:169-182 */
uint32_t mlsgpu_hip_compute_max_swathe(uint32_t yMax, uint32_t y, uint32_t yAlign, uint32_t zAlign);

/* ---- small device helpers that mirror the reference's one-work-item test kernels
 *      (kernels/octree.cl:355-372, mls.cl:439-481, marching.cl:364-371); each runs on the GPU ---- */
int mlsgpu_hip_test_make_code(mlsgpu_ctx *ctx, int x, int y, int z, uint32_t *out);
int mlsgpu_hip_test_level_shift(mlsgpu_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t *out);
int mlsgpu_hip_test_point_box_dist2(mlsgpu_ctx *ctx, const float p[3], const float lo[3], const float hi[3], float *out);
int mlsgpu_hip_test_solve_quadratic(mlsgpu_ctx *ctx, float a, float b, float c, float *out);
int mlsgpu_hip_test_fit_sphere(mlsgpu_ctx *ctx, const mlsgpu_splat *hSplats, uint32_t n, float out[5]);
int mlsgpu_hip_test_compute_key(mlsgpu_ctx *ctx, const uint32_t coords[3], const uint32_t top[3], uint64_t *out);
/* primitives: exclusive scan with seed (clogs::Scan) and stable radix sort on the low `bits` (clogs::Radixsort) */
int mlsgpu_hip_test_scan_u32(mlsgpu_ctx *ctx, uint32_t *dData, uint64_t n, uint32_t seed);
/* `repeats` scans of `count` (<= MLSGPU_MAX_BATCH) lanes each, dIn[k] -> dOut[k] (n[k] elements from seeds[k]): one set of
 * launches per repeat, as the buckets of a batch scan (src/marching.cpp:353,583,721 per bucket), back to back */
int mlsgpu_hip_test_scan_u32_batch(mlsgpu_ctx *ctx, const uint32_t *const *dIn, uint32_t *const *dOut, const uint64_t *n,
                                   const uint32_t *seeds, uint32_t count, uint32_t repeats);
int mlsgpu_hip_test_sort_u32(mlsgpu_ctx *ctx, uint32_t *dKeys, uint32_t *dValues, uint64_t n, uint32_t bits);
int mlsgpu_hip_test_sort_u64(mlsgpu_ctx *ctx, uint64_t *dKeys, uint32_t *dValues, uint64_t n, uint32_t bits);
/* The scan by element kind and form.  words: 1 scans uint32, 3 scans (a, b, c) triples of uint32 column by column (Marching's
 * cells / vertices / indices).  form: the whole scan as its callers get it (one launch up to 1 024 tiles); the scan whose tile
 * sums and prefixes are fed by two functor types (raw tile sums, then every workgroup adds up its predecessors'); or phase 1
 * (tile sums scanned by one workgroup) followed by phase 2.  dIn -> dPrefix (exclusive prefix from `seed`) and dValues (the
 * element as the consumer is handed it), n elements of `words` words each; *dTotal (`words` words on the device) = seed +
 * sum.  dCount (optional, on the device): only the first min(n, *dCount) elements exist; nothing is written behind them. */
#define MLSGPU_TEST_SCAN_WHOLE 0u
#define MLSGPU_TEST_SCAN_TWO_INPUTS 1u
#define MLSGPU_TEST_SCAN_PHASES 2u
int mlsgpu_hip_test_scan(mlsgpu_ctx *ctx, uint32_t words, uint32_t form, const uint32_t *dIn, uint32_t *dPrefix,
                         uint32_t *dValues, uint64_t n, const uint32_t seed[3], const uint32_t *dCount, uint32_t *dTotal);
/* One batched sort of `count` (<= MLSGPU_MAX_BATCH) lanes of (key, value) pairs, keys of keyBytes (4 or 8) bytes, stable on key
 * bits [doneBits, bits): lane k sorts (dKeys[k], dValues[k])[0 .. n[k]), or the first min(n[k], *dCount[k]) of them where
 * dCount (optional, as may be each of its elements) names a count on the device.  iota: the values are the positions and
 * dValues is not read.  doneBits: the input is sorted by that many low bits already.  keysWanted = 0: only the values are
 * delivered.  The temporaries and the histogram are the entry point's own; it fails if anything was written behind a
 * temporary's n[k] elements.  side[k] = 0 if lane k's result lies in dKeys[k] / dValues[k], 1 if in the temporaries; n[k]
 * elements of it are copied to dKeysOut[k] / dValuesOut[k] where those (optional, as may be each element) are given. */
int mlsgpu_hip_test_sort_batch(mlsgpu_ctx *ctx, uint32_t keyBytes, uint32_t count, void *const *dKeys, uint32_t *const *dValues,
                               const uint64_t *n, const uint32_t *const *dCount, uint32_t bits, int iota, uint32_t doneBits,
                               int keysWanted, void *const *dKeysOut, uint32_t *const *dValuesOut, uint32_t *side);

#ifdef __cplusplus
}
#endif
#endif /* MLSGPU_HIP_H */
