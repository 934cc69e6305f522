/*
 * Header-only C++ mirror of the reference's device-path classes over the C-ABI of
 * include/mlsgpu_hip.h.  Names, argument meaning and error behaviour follow the reference so that
 * code written against SplatTreeCL / MlsFunctor / Marching / DeviceWorkerGroup
 * (src/splat_tree_cl.h, src/mls.h, src/marching.h, src/mesh.h, src/mesh_filter.h, src/workers.h)
 * ports by replacing cl::Context+cl::Device with mlsgpu::hip::Context, cl::CommandQueue with the
 * context's stream, cl::Buffer with device pointers and cl::Event chains with stream order.
 *
 * Errors: MLSGPU_ERR_LENGTH -> std::length_error, MLSGPU_ERR_INVALID -> std::invalid_argument
 * (the reference's MLSGPU_ASSERT classes, src/errors.h:41-42), anything else -> mlsgpu::hip::Error
 * (the reference's cl::Error).
 */
#ifndef MLSGPU_AMD_HOST_HPP
#define MLSGPU_AMD_HOST_HPP

#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/mlsgpu_hip.h"

namespace mlsgpu
{
namespace hip
{

class Error : public std::runtime_error
{
public:
    int code;
    Error(int code, const std::string &what) : std::runtime_error(what), code(code) {}
};

inline void check(int rc)
{
    if (rc == MLSGPU_OK)
        return;
    const std::string msg = mlsgpu_hip_last_error();
    switch (rc)
    {
    case MLSGPU_ERR_LENGTH: throw std::length_error(msg);
    case MLSGPU_ERR_INVALID: throw std::invalid_argument(msg);
    default: throw Error(rc, msg);
    }
}

/// One device + one in-order stream: what a worker's cl::Context + cl::CommandQueue are in the reference.
class Context
{
    mlsgpu_ctx *h;
    Context(const Context &);
    Context &operator=(const Context &);
public:
    explicit Context(int device, void *stream = NULL) : h(NULL) { check(mlsgpu_hip_ctx_create(device, stream, &h)); }
    ~Context() { mlsgpu_hip_ctx_destroy(h); }
    mlsgpu_ctx *get() const { return h; }
    void *stream() const { return mlsgpu_hip_ctx_stream(h); }
    void finish() const { check(mlsgpu_hip_ctx_synchronize(h)); }            // cl::CommandQueue::finish
    void releaseScratch() const { check(mlsgpu_hip_ctx_release_scratch(h)); }   // what Bucket::bucket keeps between calls
    void setTiming(bool on) const { check(mlsgpu_hip_ctx_set_timing(h, on)); } // --statistics-cl
};

/// cl::Buffer
template<typename T>
class Buffer
{
    const Context *ctx;
    T *ptr;
    std::size_t count;
    Buffer(const Buffer &);
    Buffer &operator=(const Buffer &);
public:
    Buffer(const Context &ctx, std::size_t count) : ctx(&ctx), ptr(NULL), count(count)
    {
        void *p = NULL;
        check(mlsgpu_hip_malloc(ctx.get(), count * sizeof(T), &p));
        ptr = static_cast<T *>(p);
    }
    ~Buffer() { mlsgpu_hip_free(ctx->get(), ptr); }
    T *get() const { return ptr; }
    std::size_t size() const { return count; }
    void write(const T *src, std::size_t n, std::size_t first = 0, bool blocking = true) const
    {
        check(mlsgpu_hip_memcpy_h2d(ctx->get(), ptr + first, src, n * sizeof(T), !blocking));
    }
    void read(T *dst, std::size_t n, std::size_t first = 0, bool blocking = true) const
    {
        check(mlsgpu_hip_memcpy_d2h(ctx->get(), dst, ptr + first, n * sizeof(T), !blocking));
    }
};

/// namespace Manifold of test/manifold.h for a mesh in device memory
namespace Manifold
{
struct Metadata                 // test/manifold.h:53-75
{
    std::size_t numVertices, numTriangles, numComponents, numBoundaries;
    Metadata() : numVertices(0), numTriangles(0), numComponents(0), numBoundaries(0) {}
};
inline std::string reason(const mlsgpu_topology &t)
{
    char text[128];
    mlsgpu_hip_topology_reason(&t, text, sizeof(text));
    return text;
}
/// Manifold::isManifold: "" if manifold (then *data is filled), else a sentence about the first defect (*data all zero).
inline std::string isManifold(const Context &ctx, const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles,
                              std::uint64_t numVertices, Metadata *data = NULL)
{
    mlsgpu_topology t;
    check(mlsgpu_hip_mesh_topology(ctx.get(), triangles.get(), numTriangles, numVertices, &t));
    if (data != NULL)
    {
        *data = Metadata();
        if (t.manifold)
        {
            data->numVertices = t.numVertices;
            data->numTriangles = t.numTriangles;
            data->numComponents = t.numComponents;
            data->numBoundaries = t.numBoundaries;
        }
    }
    return reason(t);
}
} // namespace Manifold

/// Vertex clustering of a mesh in device memory (mlsgpu_hip_mesh_simplify): outVertices / outTriangles have room for the
/// input's sizes and do not overlap it; the result's sizes are in the returned statistics.
inline mlsgpu_simplify_stats simplify(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                      const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles, const float origin[3],
                                      float cellSize, Buffer<float> &outVertices, Buffer<std::uint32_t> &outTriangles)
{
    mlsgpu_simplify_stats st;
    check(mlsgpu_hip_mesh_simplify(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, origin, cellSize,
                                   outVertices.get(), outTriangles.get(), &st));
    return st;
}

/// simplify() with every cluster's vertex at the minimiser of its triangles' plane quadrics, which keeps the creases the mean
/// chamfers (mlsgpu_hip_mesh_simplify_quadric): the same triangles and numbering, other positions.
inline mlsgpu_simplify_quadric_stats simplifyQuadric(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                                     const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles,
                                                     const float origin[3], float cellSize, Buffer<float> &outVertices,
                                                     Buffer<std::uint32_t> &outTriangles)
{
    mlsgpu_simplify_quadric_stats st;
    check(mlsgpu_hip_mesh_simplify_quadric(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, origin, cellSize,
                                           outVertices.get(), outTriangles.get(), &st));
    return st;
}

/// Hole filling of a mesh in device memory (mlsgpu_hip_mesh_fill_holes): every boundary loop of at most maxEdges sides, none of
/// whose vertices `pinned` (NULL, or one byte per vertex) marks, gets a fan to the mean of its vertices.  outVertices /
/// outTriangles have room for capVertices / capTriangles and do not overlap the inputs; with too little room (NULL and 0 ask for
/// the sizes) nothing is written, *st is complete and std::length_error is thrown.
inline mlsgpu_fill_stats fillHoles(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                   const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles, std::uint32_t maxEdges,
                                   const std::uint8_t *pinned, float *outVertices, std::uint64_t capVertices,
                                   std::uint32_t *outTriangles, std::uint64_t capTriangles, mlsgpu_fill_stats *st = NULL)
{
    mlsgpu_fill_stats own;
    mlsgpu_fill_stats *const s = st != NULL ? st : &own;
    check(mlsgpu_hip_mesh_fill_holes(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, maxEdges, pinned,
                                     outVertices, capVertices, outTriangles, capTriangles, s));
    return *s;
}

/// The deviation report (mlsgpu_hip_mesh_deviation): the squared distance of numPoints points to the surface of a mesh, exact up
/// to maxDistance, and its statistics; everything in device memory and nothing modified.  distance2 / nearest are NULL or get
/// one entry per point (+infinity and 0xFFFFFFFF for a point beyond maxDistance).
inline mlsgpu_deviation deviation(const Context &ctx, const Buffer<float> &points, std::uint64_t numPoints,
                                  const Buffer<float> &vertices, std::uint64_t numVertices, const Buffer<std::uint32_t> &triangles,
                                  std::uint64_t numTriangles, float maxDistance, double *distance2 = NULL,
                                  std::uint32_t *nearest = NULL)
{
    mlsgpu_deviation st;
    check(mlsgpu_hip_mesh_deviation(ctx.get(), points.get(), numPoints, vertices.get(), numVertices, triangles.get(), numTriangles,
                                    maxDistance, distance2, nearest, &st));
    return st;
}

/// The self-intersection report (mlsgpu_hip_mesh_self_intersections): the pairs of triangles of a mesh in device memory that
/// certainly pass through each other -- a lower bound: touching, coplanar overlap and uncertain signs are not reported.
/// partners is NULL or gets one count per triangle; pairs is NULL or has room for pairCapacity rows (A, B) and gets the crossing
/// pairs in ascending order.  With a pairs and too little room the list stays untouched, *st is complete (when given) and
/// std::length_error is thrown: that is how to ask for the size.
inline mlsgpu_self_intersections selfIntersections(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                                   const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles,
                                                   std::uint32_t *partners = NULL, std::uint32_t *pairs = NULL,
                                                   std::uint64_t pairCapacity = 0, mlsgpu_self_intersections *st = NULL)
{
    mlsgpu_self_intersections own;
    mlsgpu_self_intersections *const s = st != NULL ? st : &own;
    check(mlsgpu_hip_mesh_self_intersections(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, partners, pairs,
                                             pairCapacity, s));
    return *s;
}

/// The compact blob of a mesh in device memory (mlsgpu_hip_mesh_compact), written to the capacityBytes of device memory at out:
/// triangles lossless, vertices bit-exact at vertexBits = 32 and quantised at 8..24.  With a NULL out or too little room nothing
/// is written, *st is complete (when given) and std::length_error is thrown: that is how to ask for the size.
inline mlsgpu_compact_stats compact(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                    const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles, std::uint32_t vertexBits,
                                    void *out, std::uint64_t capacityBytes, mlsgpu_compact_stats *st = NULL)
{
    mlsgpu_compact_stats own;
    mlsgpu_compact_stats *const s = st != NULL ? st : &own;
    check(mlsgpu_hip_mesh_compact(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, vertexBits, out, capacityBytes, s));
    return *s;
}

/// What a compact blob in host memory holds (mlsgpu_hip_compact_info): validated first, Error(MLSGPU_ERR_FORMAT) if malformed.
inline mlsgpu_compact_stats compactInfo(const void *blob, std::uint64_t bytes)
{
    mlsgpu_compact_stats st;
    check(mlsgpu_hip_compact_info(blob, bytes, &st));
    return st;
}

/// A compact blob in host memory decoded on `threads` host threads, 0 meaning 8 (mlsgpu_hip_compact_decode): no GPU involved.
inline mlsgpu_compact_stats compactDecode(const void *blob, std::uint64_t bytes, std::vector<float> &vertices,
                                          std::vector<std::uint32_t> &triangles, std::uint32_t threads = 0)
{
    const mlsgpu_compact_stats st = compactInfo(blob, bytes);
    vertices.resize(3 * st.numVertices);
    triangles.resize(3 * st.numTriangles);
    check(mlsgpu_hip_compact_decode(blob, bytes, vertices.data(), triangles.data(), threads));
    return st;
}

/// Repair of a mesh in device memory (mlsgpu_hip_mesh_repair): triangles with a repeated directed side are dropped and pinched
/// vertices split (flags: 0 or MLSGPU_REPAIR_SPLIT_PINCHES), so that the topology report calls the result manifold.
/// outVertices / outTriangles have room for capVertices / capTriangles and do not overlap the inputs; outSource is NULL or gets
/// the input index of every output vertex.  With too little room (NULL and 0 ask for the sizes) nothing is written, *st is
/// complete and std::length_error is thrown.
inline mlsgpu_repair_stats repair(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                  const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles, std::uint32_t flags,
                                  float *outVertices, std::uint64_t capVertices, std::uint32_t *outTriangles,
                                  std::uint64_t capTriangles, std::uint32_t *outSource = NULL, mlsgpu_repair_stats *st = NULL)
{
    mlsgpu_repair_stats own;
    mlsgpu_repair_stats *const s = st != NULL ? st : &own;
    check(mlsgpu_hip_mesh_repair(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, flags, outVertices,
                                 capVertices, outTriangles, capTriangles, outSource, s));
    return *s;
}

/// Taubin lambda|mu smoothing of a mesh in device memory (mlsgpu_hip_mesh_smooth): outVertices has room for 3 floats per
/// vertex and is either `vertices` itself (in place) or does not overlap the inputs.
inline mlsgpu_smooth_stats smooth(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                  const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles, std::uint32_t iterations,
                                  float lambda, float mu, std::uint32_t boundary, Buffer<float> &outVertices)
{
    mlsgpu_smooth_stats st;
    check(mlsgpu_hip_mesh_smooth(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, iterations, lambda, mu,
                                 boundary, outVertices.get(), &st));
    return st;
}

/// Delaunay edge flips of a mesh in device memory, with its quality report (mlsgpu_hip_mesh_flip_edges): outTriangles has
/// room for 3 indices per triangle and is either `triangles` itself (in place) or does not overlap the inputs.
inline mlsgpu_flip_stats flipEdges(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                   const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles, std::uint32_t maxRounds,
                                   double minGain, double minCos, Buffer<std::uint32_t> &outTriangles)
{
    mlsgpu_flip_stats st;
    check(mlsgpu_hip_mesh_flip_edges(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, maxRounds, minGain, minCos,
                                     outTriangles.get(), &st));
    return st;
}

/// Short-edge collapse of a mesh in device memory, with its quality report (mlsgpu_hip_mesh_collapse_edges): interior edges of
/// at most maxLength go, one vertex and two triangles apiece, and the topology stays.  outVertices / outTriangles have room
/// for capVertices / capTriangles and do not overlap the inputs; outSource is NULL or gets the input index of every output
/// vertex.  With too little room (NULL and 0 ask for the sizes) nothing is written, *st is complete and std::length_error is
/// thrown.
inline mlsgpu_collapse_stats collapseEdges(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                           const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles,
                                           std::uint32_t maxRounds, double maxLength, double minCos, float *outVertices,
                                           std::uint64_t capVertices, std::uint32_t *outTriangles, std::uint64_t capTriangles,
                                           std::uint32_t *outSource = NULL, mlsgpu_collapse_stats *st = NULL)
{
    mlsgpu_collapse_stats own;
    mlsgpu_collapse_stats *const s = st != NULL ? st : &own;
    check(mlsgpu_hip_mesh_collapse_edges(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, maxRounds, maxLength,
                                         minCos, outVertices, capVertices, outTriangles, capTriangles, outSource, s));
    return *s;
}

/// Long-edge split of a mesh in device memory, with its quality report (mlsgpu_hip_mesh_split_edges): every edge above
/// maxLength that is the longest side of its triangles is halved, round after round; maxOutTriangles (0: none) stops the
/// rounds before the one that would pass it, pinned is NULL or one byte per input vertex.  outVertices / outTriangles have
/// room for capVertices / capTriangles and do not overlap the inputs; outEnds is NULL or gets the two ends of every new
/// vertex's edge.  With too little room (NULL and 0 ask for the sizes) nothing is written, *st is complete and
/// std::length_error is thrown.
inline mlsgpu_split_stats splitEdges(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                     const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles, std::uint32_t maxRounds,
                                     double maxLength, std::uint64_t maxOutTriangles, const std::uint8_t *pinned, float *outVertices,
                                     std::uint64_t capVertices, std::uint32_t *outTriangles, std::uint64_t capTriangles,
                                     std::uint32_t *outEnds = NULL, mlsgpu_split_stats *st = NULL)
{
    mlsgpu_split_stats own;
    mlsgpu_split_stats *const s = st != NULL ? st : &own;
    check(mlsgpu_hip_mesh_split_edges(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, maxRounds, maxLength,
                                      maxOutTriangles, pinned, outVertices, capVertices, outTriangles, capTriangles, outEnds, s));
    return *s;
}

/// Area-weighted vertex normals of a mesh in device memory (mlsgpu_hip_mesh_normals): outNormals has room for 3 floats per
/// vertex and does not overlap the inputs.
inline mlsgpu_normals_stats normals(const Context &ctx, const Buffer<float> &vertices, std::uint64_t numVertices,
                                    const Buffer<std::uint32_t> &triangles, std::uint64_t numTriangles, Buffer<float> &outNormals)
{
    mlsgpu_normals_stats st;
    check(mlsgpu_hip_mesh_normals(ctx.get(), vertices.get(), numVertices, triangles.get(), numTriangles, outNormals.get(), &st));
    return st;
}

typedef mlsgpu_splat Splat;                 // src/splat.h:40-46
enum MlsShape { MLS_SHAPE_SPHERE = MLSGPU_SHAPE_SPHERE, MLS_SHAPE_PLANE = MLSGPU_SHAPE_PLANE };  // src/mls.h:47-51

/// SplatTreeCL, src/splat_tree_cl.h:216-296
class SplatTreeCL
{
    mlsgpu_tree *h;
    SplatTreeCL(const SplatTreeCL &);
    SplatTreeCL &operator=(const SplatTreeCL &);
public:
    typedef std::int32_t command_type;
    enum { MAX_LEVELS = MLSGPU_TREE_MAX_LEVELS };
    static std::uint64_t resourceUsage(std::size_t maxLevels, std::size_t maxSplats)
    {
        return mlsgpu_hip_tree_resource_usage(maxLevels, maxSplats);
    }
    SplatTreeCL(const Context &ctx, std::size_t maxLevels, std::size_t maxSplats) : h(NULL)
    {
        check(mlsgpu_hip_tree_create(ctx.get(), maxLevels, maxSplats, &h));
    }
    ~SplatTreeCL() { mlsgpu_hip_tree_destroy(h); }
    /// src/splat_tree_cl.cpp:269-335.  Ordering is the context's stream instead of cl::Event lists.
    void enqueueBuild(Splat *splats, std::size_t firstSplat, std::size_t numSplats,
                      const std::uint32_t size[3], const std::int32_t offset[3], unsigned int subsamplingShift)
    {
        check(mlsgpu_hip_tree_build(h, splats, firstSplat, numSplats, size, offset, subsamplingShift));
    }
    void clearSplats() { mlsgpu_hip_tree_clear_splats(h); }
    /* false: enqueueBuild leaves the splats untouched (no radius -> 1/radius^2); MlsFunctor::set follows the tree */
    void setMutate(bool mutate) { check(mlsgpu_hip_tree_set_mutate(h, mutate ? 1 : 0)); }
    const Splat *getSplats() const { return mlsgpu_hip_tree_splats(h); }
    const command_type *getCommands() const { return mlsgpu_hip_tree_commands(h); }
    const command_type *getStart() const { return mlsgpu_hip_tree_start(h); }
    std::size_t getNumLevels() const { return mlsgpu_hip_tree_num_levels(h); }
    mlsgpu_tree *get() const { return h; }
};

/// MeshSizes / DeviceKeyMesh / HostKeyMesh, src/mesh.h:40-179
struct DeviceKeyMesh : public mlsgpu_mesh
{
    std::size_t numExternalVertices() const { return numVertices - numInternalVertices; }
    std::size_t getHostBytes() const { return mlsgpu_hip_mesh_host_bytes(this); }
};

struct HostKeyMesh
{
    std::uint64_t *vertexKeys;      // numExternalVertices entries: vertexKeys[i] belongs to vertices[i + numInternal]
    float (*vertices)[3];
    std::uint32_t (*triangles)[3];
    std::size_t numVertices, numTriangles, numInternalVertices;

    /// Construct over an existing 8-byte aligned pool of getHostBytes() bytes (src/mesh.cpp:51-60).
    HostKeyMesh(void *ptr, const DeviceKeyMesh &sizes)
        : numVertices(sizes.numVertices), numTriangles(sizes.numTriangles), numInternalVertices(sizes.numInternalVertices)
    {
        if (reinterpret_cast<std::uintptr_t>(ptr) % 8 != 0)
            throw std::invalid_argument("HostKeyMesh: pointer is not 8-byte aligned");
        vertexKeys = static_cast<std::uint64_t *>(ptr);
        vertices = reinterpret_cast<float (*)[3]>(vertexKeys + (numVertices - numInternalVertices));
        triangles = reinterpret_cast<std::uint32_t (*)[3]>(vertices + numVertices);
    }
};

/// enqueueReadMesh, src/mesh.cpp:62-102: all three arrays, asynchronous on the context's stream.
inline void enqueueReadMesh(const Context &ctx, const DeviceKeyMesh &dMesh, HostKeyMesh &hMesh)
{
    check(mlsgpu_hip_mesh_read(ctx.get(), &dMesh, hMesh.vertexKeys, 1));
}

/// Marching, src/marching.h:204-608
class Marching
{
    mlsgpu_marching *h;
    Marching(const Marching &);
    Marching &operator=(const Marching &);
public:
    enum { MAX_CELL_BYTES = MLSGPU_MARCHING_MAX_CELL_BYTES, MAX_DIMENSION = MLSGPU_MARCHING_MAX_DIMENSION };
    typedef mlsgpu_swathe Swathe;

    /// Marching::Generator, src/marching.h:204-253
    class Generator
    {
    public:
        virtual ~Generator() {}
        virtual const std::uint32_t *alignment() const = 0;
        /// Enqueue work on `stream` that fills slices swathe.zFirst..zLast of `distance`
        /// (corner (x,y,z) at distance[(y + z*zStride + zBias) * pitch + x]).
        virtual void enqueue(void *stream, float *distance, std::size_t pitch, const Swathe &swathe) = 0;
    };

    /// Marching::OutputFunctor, src/marching.h:516-546
    typedef std::function<void(void *stream, const DeviceKeyMesh &mesh)> OutputFunctor;

    static std::uint64_t resourceUsage(std::uint32_t maxWidth, std::uint32_t maxHeight, std::uint32_t maxDepth,
                                       std::uint32_t maxSwathe, std::size_t meshMemory, const std::uint32_t alignment[3])
    {
        return mlsgpu_hip_marching_resource_usage(maxWidth, maxHeight, maxDepth, maxSwathe, meshMemory, alignment);
    }

    Marching(const Context &ctx, std::uint32_t maxWidth, std::uint32_t maxHeight, std::uint32_t maxDepth,
             std::uint32_t maxSwathe, std::size_t meshMemory, const std::uint32_t alignment[3]) : h(NULL)
    {
        check(mlsgpu_hip_marching_create(ctx.get(), maxWidth, maxHeight, maxDepth, maxSwathe, meshMemory, alignment, &h));
    }
    ~Marching() { mlsgpu_hip_marching_destroy(h); }

    /// src/marching.cpp:745-824.  Blocks until the bucket is finished, like the reference.
    void generate(Generator &generator, const OutputFunctor &output,
                  const std::uint32_t size[3], const std::uint32_t keyOffset[3])
    {
        Thunk thunk = {&generator, &output, std::exception_ptr()};
        mlsgpu_generator g;
        const std::uint32_t *a = generator.alignment();
        g.alignment[0] = a[0]; g.alignment[1] = a[1]; g.alignment[2] = a[2];
        g.enqueue = &Marching::enqueueThunk;
        g.user = &thunk;
        const int rc = mlsgpu_hip_marching_generate(h, &g, &Marching::outputThunk, &thunk, size, keyOffset);
        if (thunk.error)
            std::rethrow_exception(thunk.error);
        check(rc);
    }
    mlsgpu_marching *get() const { return h; }

private:
    struct Thunk
    {
        Generator *generator;
        const OutputFunctor *output;
        std::exception_ptr error;
    };
    static int enqueueThunk(void *user, void *stream, float *field, std::uint64_t pitch, const mlsgpu_swathe *sw)
    {
        Thunk *t = static_cast<Thunk *>(user);
        try { t->generator->enqueue(stream, field, pitch, *sw); return 0; }
        catch (...) { t->error = std::current_exception(); return MLSGPU_ERR_CALLBACK; }
    }
    static int outputThunk(void *user, void *stream, const mlsgpu_mesh *mesh)
    {
        Thunk *t = static_cast<Thunk *>(user);
        try { (*t->output)(stream, *static_cast<const DeviceKeyMesh *>(mesh)); return 0; }
        catch (...) { t->error = std::current_exception(); return MLSGPU_ERR_CALLBACK; }
    }
};

/// MlsFunctor, src/mls.h:79-170
class MlsFunctor : public Marching::Generator
{
    mlsgpu_mls *h;
    std::uint32_t wgs_[3];
public:
    static const int subsamplingMin = 3;
    MlsFunctor(const Context &ctx, MlsShape shape) : h(NULL)
    {
        check(mlsgpu_hip_mls_create(ctx.get(), shape, &h));
        wgs_[0] = wgs_[1] = wgs_[2] = 8;      // MlsFunctor::wgs, src/mls.cpp:53
    }
    ~MlsFunctor() { mlsgpu_hip_mls_destroy(h); }
    void set(const std::int32_t offset[3], const SplatTreeCL &tree, unsigned int subsamplingShift)
    {
        check(mlsgpu_hip_mls_set(h, offset, tree.get(), subsamplingShift));
    }
    void setBoundaryLimit(float limit) { check(mlsgpu_hip_mls_set_boundary_limit(h, limit)); }
    /* with explicit buffers: the splats still hold the radius, not 1/radius^2 */
    void setRawRadius(bool raw) { check(mlsgpu_hip_mls_set_raw_radius(h, raw ? 1 : 0)); }
    virtual const std::uint32_t *alignment() const { return wgs_; }
    virtual void enqueue(void *, float *distance, std::size_t pitch, const Marching::Swathe &swathe)
    {
        check(mlsgpu_hip_mls_enqueue(h, distance, pitch, UINT64_MAX, &swathe));
    }
    mlsgpu_mls *get() const { return h; }
};

/// ScaleBiasFilter, src/mesh_filter.h:117-168 (in place; returns its input like the reference's outMesh = inMesh)
class ScaleBiasFilter
{
    const Context *ctx;
    float scale, bias[3];
public:
    explicit ScaleBiasFilter(const Context &ctx) : ctx(&ctx), scale(1.0f) { bias[0] = bias[1] = bias[2] = 0.0f; }
    void setScaleBias(float s, float x, float y, float z) { scale = s; bias[0] = x; bias[1] = y; bias[2] = z; }
    void operator()(void *, const DeviceKeyMesh &inMesh, DeviceKeyMesh &outMesh) const
    {
        check(mlsgpu_hip_scale_bias(ctx->get(), &inMesh, scale, bias[0], bias[1], bias[2]));
        outMesh = inMesh;
    }
};

/// MeshFilterChain, src/mesh_filter.h:69-115
class MeshFilterChain
{
public:
    typedef std::function<void(void *stream, const DeviceKeyMesh &in, DeviceKeyMesh &out)> Filter;
    void addFilter(const Filter &f) { filters.push_back(f); }
    void setOutput(const Marching::OutputFunctor &o) { output = o; }
    void operator()(void *stream, const DeviceKeyMesh &mesh) const      // src/mesh_filter.cpp:45-66
    {
        DeviceKeyMesh a = mesh, b;
        for (std::size_t i = 0; i < filters.size(); i++)
        {
            filters[i](stream, a, b);
            a = b;
        }
        output(stream, a);
    }
private:
    std::vector<Filter> filters;
    Marching::OutputFunctor output;
};

/// A bucket grid: low extents + number of vertices per axis (the part of Grid the worker reads,
/// src/workers.cpp:237-261) and the full grid's spacing / origin for ScaleBiasFilter (:227-230).
struct BucketGrid
{
    std::int32_t low[3];
    std::uint32_t numVertices[3];
};

/**
 * DeviceWorkerGroup, src/workers.h:214-350 / src/workers.cpp:87-286, re-expressed with std::thread:
 * `numWorkers` threads, each owning a Context (stream) and an mlsgpu_worker (tree + MlsFunctor +
 * Marching + ScaleBias), fed from a pool of numWorkers + spare device splat buffers.  The producer calls
 * get() for an item, fills item->splats (its own H2D copy on item->copyStream or via write()), lists
 * the buckets in item->subItems and push()es it.
 */
class DeviceWorkerGroup
{
public:
    struct SubItem              // src/workers.h:148-160
    {
        std::uint64_t chunkId;
        BucketGrid grid;
        std::size_t firstSplat, numSplats, progressSplats;
    };
    struct WorkItem             // src/workers.h:165-181
    {
        std::vector<SubItem> subItems;
        std::unique_ptr<Buffer<Splat> > splats;
        std::size_t numSplats() const
        {
            std::size_t n = 0;
            for (std::size_t i = 0; i < subItems.size(); i++) n += subItems[i].numSplats;
            return n;
        }
    };
    /// OutputGenerator, src/workers.h:225: makes the output functor for one chunk.
    typedef std::function<Marching::OutputFunctor(std::uint64_t chunkId)> OutputGenerator;

    DeviceWorkerGroup(std::size_t numWorkers, std::size_t spare, const OutputGenerator &outputGenerator, int device,
                      std::size_t maxBucketSplats, std::uint32_t maxCells, std::size_t meshMemory,
                      int levels, int subsampling, float boundaryLimit, MlsShape shape)
        : outputGenerator(outputGenerator), device(device), maxItemSplats(maxBucketSplats), stopping(false),
          unallocated_(0), itemCtx(device)
    {
        std::memset(&cfg, 0, sizeof(cfg));
        cfg.maxBucketSplats = maxBucketSplats;
        cfg.maxCells = maxCells;
        cfg.meshMemory = meshMemory;
        cfg.levels = levels;
        cfg.subsampling = subsampling;
        cfg.boundaryLimit = boundaryLimit;
        cfg.shape = shape;
        cfg.gridSpacing = 1.0f;
        for (std::size_t i = 0; i < numWorkers + spare; i++)
        {
            std::shared_ptr<WorkItem> item(new WorkItem);
            item->splats.reset(new Buffer<Splat>(itemCtx, maxItemSplats));
            itemPool.push_back(item);
        }
        unallocated_ = maxItemSplats * (numWorkers + spare);
        this->numWorkers = numWorkers;
    }
    ~DeviceWorkerGroup() { if (!threads.empty()) stop(); }

    /// src/workers.cpp:184-205.  `lanes`: what setBatch() will be given -- every worker then holds that many sets of tree,
    /// field, lattice and mesh arena.
    static std::uint64_t resourceUsage(std::size_t numWorkers, std::size_t spare, std::size_t maxBucketSplats,
                                       std::uint32_t maxCells, std::size_t meshMemory, int levels, std::uint32_t lanes = 1)
    {
        mlsgpu_worker_config c;
        std::memset(&c, 0, sizeof(c));
        c.maxBucketSplats = maxBucketSplats; c.maxCells = maxCells; c.meshMemory = meshMemory; c.levels = levels;
        return mlsgpu_hip_worker_resource_usage_lanes(&c, lanes) * numWorkers
            + maxBucketSplats * sizeof(Splat) * (numWorkers + spare);
    }

    /// start(fullGrid): spacing and world position of vertex (0,0,0) feed ScaleBiasFilter (src/workers.cpp:124-128,227-230)
    void start(float gridSpacing, const float gridOrigin[3])
    {
        cfg.gridSpacing = gridSpacing;
        for (int i = 0; i < 3; i++) cfg.gridOrigin[i] = gridOrigin[i];
        for (std::size_t i = 0; i < numWorkers; i++)
            threads.push_back(std::thread(&DeviceWorkerGroup::run, this));
    }
    /// Buckets of a work item the workers take through the device path in lock-step (1 .. MLSGPU_MAX_BATCH; default 1 =
    /// the reference's loop over the SubItems, src/workers.cpp:232-286).  Before start(); the outputs do not change.
    void setBatch(std::uint32_t lanes) { batch = lanes; }
    /// of a batch's buckets, how many share one set of processCorners / marching launches (0: all; the octree takes the batch)
    void setMarchingGroup(std::uint32_t buckets) { marchingGroup = buckets; }
    bool canGet() { std::lock_guard<std::mutex> l(mutex); return !itemPool.empty(); }
    std::shared_ptr<WorkItem> get(std::size_t numSplats)                    // src/workers.cpp:135-146
    {
        std::unique_lock<std::mutex> l(mutex);
        poolCond.wait(l, [this] { return !itemPool.empty(); });
        std::shared_ptr<WorkItem> item = itemPool.front();
        itemPool.pop_front();
        unallocated_ -= numSplats;
        return item;
    }
    void push(const std::shared_ptr<WorkItem> &item)
    {
        itemCtx.finish();        // the producer's writes through item->splats are complete
        { std::lock_guard<std::mutex> l(mutex); queue.push_back(item); }
        queueCond.notify_one();
    }
    std::size_t unallocated() { std::lock_guard<std::mutex> l(mutex); return unallocated_; }   // src/workers.cpp:163-167
    std::size_t getMaxItemSplats() const { return maxItemSplats; }
    void stop()
    {
        { std::lock_guard<std::mutex> l(mutex); stopping = true; }
        queueCond.notify_all();
        for (std::size_t i = 0; i < threads.size(); i++) threads[i].join();
        threads.clear();
        if (workerError)
            std::rethrow_exception(workerError);
    }

private:
    void freeItem(const std::shared_ptr<WorkItem> &item)                    // src/workers.cpp:148-161
    {
        item->subItems.clear();
        { std::lock_guard<std::mutex> l(mutex); itemPool.push_back(item); }
        poolCond.notify_one();
    }
    struct OutputUser { const MeshFilterChain *chain; std::exception_ptr error; };
    struct BatchUser { std::vector<MeshFilterChain> chains; std::exception_ptr error; };
    static int batchThunk(void *user, std::uint32_t index, void *stream, const mlsgpu_mesh *mesh)
    {
        BatchUser *u = static_cast<BatchUser *>(user);
        try { u->chains[index](stream, *static_cast<const DeviceKeyMesh *>(mesh)); return 0; }
        catch (...) { u->error = std::current_exception(); return MLSGPU_ERR_CALLBACK; }
    }
    static int outputThunk(void *user, void *stream, const mlsgpu_mesh *mesh)
    {
        OutputUser *u = static_cast<OutputUser *>(user);
        try { (*u->chain)(stream, *static_cast<const DeviceKeyMesh *>(mesh)); return 0; }
        catch (...) { u->error = std::current_exception(); return MLSGPU_ERR_CALLBACK; }
    }
    void run()                                                              // Worker::operator(), src/workers.cpp:232-286
    {
        try
        {
            Context ctx(device);
            mlsgpu_worker *w = NULL;
            check(mlsgpu_hip_worker_create(ctx.get(), &cfg, &w));
            std::shared_ptr<mlsgpu_worker> guard(w, mlsgpu_hip_worker_destroy);
            if (batch > 1)
                check(mlsgpu_hip_worker_set_batch(w, batch));
            check(mlsgpu_hip_worker_set_marching_group(w, marchingGroup));
            for (;;)
            {
                std::shared_ptr<WorkItem> item;
                {
                    std::unique_lock<std::mutex> l(mutex);
                    queueCond.wait(l, [this] { return stopping || !queue.empty(); });
                    if (queue.empty())
                        return;
                    item = queue.front();
                    queue.pop_front();
                }
                if (batch > 1 && item->subItems.size() > 1)
                {
                    // the SubItems `batch` at a time through one set of launches (mlsgpu_hip_worker_process_batch)
                    BatchUser user;
                    std::vector<mlsgpu_subitem> subs(item->subItems.size());
                    user.chains.resize(subs.size());
                    std::size_t splats = 0;
                    for (std::size_t i = 0; i < subs.size(); i++)
                    {
                        const SubItem &sub = item->subItems[i];
                        user.chains[i].setOutput(outputGenerator(sub.chunkId));
                        subs[i].firstSplat = sub.firstSplat;
                        subs[i].numSplats = sub.numSplats;
                        for (int a = 0; a < 3; a++)
                        {
                            subs[i].lowExtent[a] = sub.grid.low[a];
                            subs[i].numVertices[a] = sub.grid.numVertices[a];
                        }
                        subs[i].dSplats = NULL;
                        splats += sub.numSplats;
                    }
                    const int rc = mlsgpu_hip_worker_process_batch(w, item->splats->get(), subs.data(), (std::uint32_t) subs.size(),
                                                                   &batchThunk, &user);
                    if (user.error)
                        std::rethrow_exception(user.error);
                    check(rc);
                    std::lock_guard<std::mutex> l(mutex);
                    unallocated_ += splats;
                }
                else
                for (std::size_t i = 0; i < item->subItems.size(); i++)
                {
                    const SubItem &sub = item->subItems[i];
                    MeshFilterChain chain;      // scale/bias is applied inside the worker; the chain carries the output
                    chain.setOutput(outputGenerator(sub.chunkId));
                    OutputUser user = {&chain, std::exception_ptr()};
                    const int rc = mlsgpu_hip_worker_process(w, item->splats->get(), sub.firstSplat, sub.numSplats,
                                                             sub.grid.low, sub.grid.numVertices, &outputThunk, &user);
                    if (user.error)
                        std::rethrow_exception(user.error);
                    check(rc);
                    std::lock_guard<std::mutex> l(mutex);
                    unallocated_ += sub.numSplats;
                }
                freeItem(item);
            }
        }
        catch (...)
        {
            // the reference prints and exits (src/worker_group.h:286-290); here the error surfaces from stop()
            std::lock_guard<std::mutex> l(mutex);
            if (!workerError)
                workerError = std::current_exception();
            stopping = true;
            queueCond.notify_all();
        }
    }

    OutputGenerator outputGenerator;
    int device;
    mlsgpu_worker_config cfg;
    std::size_t maxItemSplats, numWorkers;
    std::uint32_t batch = 1;
    std::uint32_t marchingGroup = 2;
    bool stopping;
    std::size_t unallocated_;
    Context itemCtx;
    std::mutex mutex;
    std::condition_variable queueCond, poolCond;
    std::deque<std::shared_ptr<WorkItem> > queue, itemPool;
    std::vector<std::thread> threads;
    std::exception_ptr workerError;
};

/**
 * MesherBase / OOCMesher (src/mesher.h:203-420) for meshes that stay on the device: functor() gives the
 * Marching::OutputFunctor that appends a ship-out, write() welds, prunes and writes one PLY per non-empty chunk.
 * One pass (numPasses() == 1).  The namer maps a chunk id to a file name (TrivialNamer / ChunkNamer, :136-182).
 */
class DeviceMesher
{
    mlsgpu_mesher *h;
    const Context *ctx;
    DeviceMesher(const DeviceMesher &);
    DeviceMesher &operator=(const DeviceMesher &);
public:
    typedef std::function<std::string(std::uint64_t chunkId)> Namer;

    explicit DeviceMesher(const Context &ctx) : h(NULL), ctx(&ctx) { check(mlsgpu_hip_mesher_create(ctx.get(), &h)); }
    ~DeviceMesher() { mlsgpu_hip_mesher_destroy(h); }
    mlsgpu_mesher *get() const { return h; }
    unsigned int numPasses() const { return 1; }
    void setPruneThreshold(double threshold) { check(mlsgpu_hip_mesher_set_prune_threshold(h, threshold)); }
    void reserve(std::uint64_t vertices, std::uint64_t triangles, std::uint64_t external)
    {
        check(mlsgpu_hip_mesher_reserve(h, vertices, triangles, external));
    }
    /// The output functor of one chunk for the worker that owns `from` (thread safe across workers).
    Marching::OutputFunctor functor(const Context &from, std::uint64_t chunkId)
    {
        mlsgpu_mesher *mesher = h;
        mlsgpu_ctx *fromCtx = from.get();
        return [mesher, fromCtx, chunkId](void *, const DeviceKeyMesh &mesh) { check(mlsgpu_hip_mesher_add(mesher, fromCtx, chunkId, &mesh)); };
    }
    /// pinned host memory a write may hold (two buffers of half this; 0 = 64 MiB), whatever the size of the mesh
    std::uint64_t writeBufferBytes = 0;
    /// The first half of write(): weld, components, prune.  Returns the number of output chunks.
    std::size_t finalize()
    {
        std::uint32_t chunks = 0;
        check(mlsgpu_hip_mesher_finalize(h, &chunks));
        return chunks;
    }
    /// Every output chunk of the finalized mesher replaced by its vertex-clustered mesh (mlsgpu_hip_mesher_simplify);
    /// between finalize() and writeChunks().  The statistics are summed over the chunks.
    mlsgpu_simplify_stats simplify(const float origin[3], float cellSize)
    {
        mlsgpu_simplify_stats st;
        check(mlsgpu_hip_mesher_simplify(h, origin, cellSize, &st));
        return st;
    }
    /// simplify() with quadric-error vertex placement (mlsgpu_hip_mesher_simplify_quadric); counts summed over the chunks, the
    /// scale's exponent the largest.
    mlsgpu_simplify_quadric_stats simplifyQuadric(const float origin[3], float cellSize)
    {
        mlsgpu_simplify_quadric_stats st;
        check(mlsgpu_hip_mesher_simplify_quadric(h, origin, cellSize, &st));
        return st;
    }
    /// Every output chunk of the finalized mesher with its boundary loops of at most maxEdges sides capped
    /// (mlsgpu_hip_mesher_fill_holes); directly behind finalize(), before simplify() and smooth(), which un-match the seams
    /// between the chunks that this call leaves open.  Counts summed over the chunks, longestLoop and exponent the largest.
    mlsgpu_fill_stats fillHoles(std::uint32_t maxEdges)
    {
        mlsgpu_fill_stats st;
        check(mlsgpu_hip_mesher_fill_holes(h, maxEdges, &st));
        return st;
    }
    /// Keeps a copy of every chunk of the finalized mesher as it is now (mlsgpu_hip_mesher_keep_reference), for deviation() to
    /// measure against: directly behind finalize(), before a stage that moves vertices.
    void keepReference() { check(mlsgpu_hip_mesher_keep_reference(h)); }
    void dropReference() { check(mlsgpu_hip_mesher_drop_reference(h)); }
    /// How far the chunks are from the kept reference (mlsgpu_hip_mesher_deviation): first the current vertices against the kept
    /// surface ("moved"), second the kept vertices against the current surface ("lost").  Changes nothing.
    std::pair<mlsgpu_deviation, mlsgpu_deviation> deviation(float maxDistance)
    {
        std::pair<mlsgpu_deviation, mlsgpu_deviation> st;
        check(mlsgpu_hip_mesher_deviation(h, maxDistance, &st.first, &st.second));
        return st;
    }
    /// The triangle pairs of each chunk that certainly pass through each other (mlsgpu_hip_mesher_self_intersections), added up
    /// over the chunks; pairs across chunks are not looked for.  Changes nothing.
    mlsgpu_self_intersections selfIntersections()
    {
        mlsgpu_self_intersections st;
        check(mlsgpu_hip_mesher_self_intersections(h, &st));
        return st;
    }
    /// Output chunk i as a compact blob in host memory (mlsgpu_hip_mesher_chunk_compact): encoded where the chunk lies, one copy
    /// across.  One call asks for the size, the second fills `blob`.  Changes nothing.
    mlsgpu_compact_stats chunkCompact(std::uint32_t i, std::uint32_t vertexBits, std::vector<std::uint32_t> &blob)
    {
        mlsgpu_compact_stats st;
        const int rc = mlsgpu_hip_mesher_chunk_compact(h, i, vertexBits, NULL, 0, &st);
        if (rc != MLSGPU_ERR_LENGTH)        // the size query ends in the length error
            check(rc);
        blob.resize(st.blobBytes / 4);
        check(mlsgpu_hip_mesher_chunk_compact(h, i, vertexBits, blob.data(), st.blobBytes, &st));
        return st;
    }
    /// Every output chunk of the finalized mesher repaired (mlsgpu_hip_mesher_repair): triangles with a repeated side dropped,
    /// pinched vertices split, so that chunk topology reports are manifold again; behind simplify(), before smooth() and
    /// writeChunks().  flags: 0 or MLSGPU_REPAIR_SPLIT_PINCHES.  The statistics are summed over the chunks.
    mlsgpu_repair_stats repair(std::uint32_t flags = 0)
    {
        mlsgpu_repair_stats st;
        check(mlsgpu_hip_mesher_repair(h, flags, &st));
        return st;
    }
    /// Every output chunk of the finalized mesher with its interior edges of at most maxLength collapsed
    /// (mlsgpu_hip_mesher_collapse_edges): behind simplify() and repair(), before flipEdges() and smooth().  The chunks move into
    /// new arrays; seams keep their bits.  Counts and histograms summed over the chunks, rounds the largest, converged the AND,
    /// the minima the minima.
    mlsgpu_collapse_stats collapseEdges(std::uint32_t maxRounds, double maxLength, double minCos = 0.5)
    {
        mlsgpu_collapse_stats st;
        check(mlsgpu_hip_mesher_collapse_edges(h, maxRounds, maxLength, minCos, &st));
        return st;
    }
    /// Every output chunk of the finalized mesher with its edges above maxLength halved, longest first
    /// (mlsgpu_hip_mesher_split_edges): behind fillHoles(), simplify() and repair(), before collapseEdges(), flipEdges() and
    /// smooth().  A chunk stops before the round that would take it above maxGrowth times its triangles (0: no limit).  The
    /// chunks grow into new arrays; with several chunks the seams are pinned and keep their bits.  Counts and histograms summed
    /// over the chunks, rounds the largest, converged the AND, limited the OR, the minima the minima, the maxima the maxima.
    mlsgpu_split_stats splitEdges(std::uint32_t maxRounds, double maxLength, std::uint32_t maxGrowth = 0)
    {
        mlsgpu_split_stats st;
        check(mlsgpu_hip_mesher_split_edges(h, maxRounds, maxLength, maxGrowth, &st));
        return st;
    }
    /// Every output chunk of the finalized mesher through at most maxRounds rounds of Delaunay edge flips, in place
    /// (mlsgpu_hip_mesher_flip_edges): triangles only, behind repair() and before smooth().  Counts and histograms summed over
    /// the chunks, rounds the largest, converged the AND, the minima the minima.
    mlsgpu_flip_stats flipEdges(std::uint32_t maxRounds, double minGain = 1e-6, double minCos = 0.5)
    {
        mlsgpu_flip_stats st;
        check(mlsgpu_hip_mesher_flip_edges(h, maxRounds, minGain, minCos, &st));
        return st;
    }
    /// Every output chunk of the finalized mesher smoothed in place (mlsgpu_hip_mesher_smooth); between finalize() -- or
    /// simplify() -- and writeChunks().  Counts summed over the chunks, exponent and maxima the largest.
    mlsgpu_smooth_stats smooth(std::uint32_t iterations, float lambda = 0.5f, float mu = -0.53f,
                               std::uint32_t boundary = MLSGPU_SMOOTH_BOUNDARY_FIXED)
    {
        mlsgpu_smooth_stats st;
        check(mlsgpu_hip_mesher_smooth(h, iterations, lambda, mu, boundary, &st));
        return st;
    }
    /// The second half of write(): one file per chunk of the `chunks` that finalize() reported; withNormals: the files of
    /// writePlyNormals().
    std::size_t writeChunks(std::size_t chunks, const Namer &namer, const std::vector<std::string> &comments = std::vector<std::string>(),
                            bool withNormals = false)
    {
        std::vector<const char *> cstr;
        for (const std::string &c : comments)
            cstr.push_back(c.c_str());
        for (std::uint32_t i = 0; i < chunks; i++)
        {
            std::uint64_t id, nv, nt;
            const float *dV;
            const std::uint32_t *dT;
            check(mlsgpu_hip_mesher_chunk(h, i, &id, &nv, &nt, &dV, &dT));
            // straight from HBM through a bounded pinned buffer (the reference's asynchronous writer, src/async_io.h)
            check((withNormals ? mlsgpu_hip_mesher_write_ply_normals : mlsgpu_hip_mesher_write_ply)(
                h, i, namer(id).c_str(), cstr.empty() ? NULL : cstr.data(), (std::uint32_t) cstr.size(), writeBufferBytes));
        }
        return chunks;
    }
    /// writeChunks() with every chunk's area-weighted vertex normals (normals(i)) as nx ny nz after z.
    std::size_t writePlyNormals(std::size_t chunks, const Namer &namer, const std::vector<std::string> &comments = std::vector<std::string>())
    {
        return writeChunks(chunks, namer, comments, true);
    }
    /// MesherBase::write: returns the number of files written.
    std::size_t write(const Namer &namer, const std::vector<std::string> &comments = std::vector<std::string>())
    {
        return writeChunks(finalize(), namer, comments);
    }
    void getStatistics(std::uint64_t out[8]) const { check(mlsgpu_hip_mesher_stats(h, out)); }
    /// The topology report of output chunk i of the last write(), computed on the device (Manifold::reason words it).
    mlsgpu_topology topology(std::uint32_t i) const
    {
        mlsgpu_topology t;
        check(mlsgpu_hip_mesher_chunk_topology(h, i, &t));
        return t;
    }
    /// The area-weighted vertex normals of output chunk i (mlsgpu_hip_mesher_chunk_normals): computed on the device at the
    /// first request, kept beside the vertices until the next finalize() or simplify(); *dNormals is 3 floats per vertex.
    mlsgpu_normals_stats normals(std::uint32_t i, const float **dNormals = NULL) const
    {
        mlsgpu_normals_stats st;
        check(mlsgpu_hip_mesher_chunk_normals(h, i, dNormals, &st));
        return st;
    }
};

/**
 * OOCMesher (src/mesher.h:331-420, src/mesher.cpp:220-469) in host memory: the reference's weld, run where the reference
 * runs it.  add() is MesherBase::InputFunctor for a HostKeyMesh; meshes of any GPU may be added (it is what
 * BucketFarm::setHostOutput feeds from its mesher thread).  write() welds, prunes and writes one PLY per non-empty
 * chunk, like DeviceMesher::write.
 */
class OOCMesher
{
    mlsgpu_host_mesher *h;
    OOCMesher(const OOCMesher &);
    OOCMesher &operator=(const OOCMesher &);
public:
    typedef std::function<std::string(std::uint64_t chunkId)> Namer;
    OOCMesher() : h(NULL) { check(mlsgpu_hip_host_mesher_create(&h)); }
    ~OOCMesher() { mlsgpu_hip_host_mesher_destroy(h); }
    mlsgpu_host_mesher *get() const { return h; }
    void setPruneThreshold(double t) { check(mlsgpu_hip_host_mesher_set_prune_threshold(h, t)); }
    /// threads of the welder (0 = default); before the first add
    void setThreads(std::uint32_t threads) { check(mlsgpu_hip_host_mesher_set_threads(h, threads)); }
    /// the welder's threads on one NUMA node (the one its meshes arrive on); -1 = unbound.  Before the first add.
    void setNode(int node) { check(mlsgpu_hip_host_mesher_set_node(h, node)); }
    int node() const { return mlsgpu_hip_host_mesher_node(h); }
    /// the reference's --tmp-dir (TmpWriterWorkerGroup, src/mesher.cpp:404-419): blocks live in temporary files there and
    /// leave memory once welded, beyond `residentBytes` of them.  Before the first add.
    void setTmpDir(const std::string &dir, std::uint64_t residentBytes = 0)
    {
        check(mlsgpu_hip_host_mesher_set_tmp_dir(h, dir.c_str(), residentBytes));
    }
    void add(std::uint64_t chunkId, const mlsgpu_host_mesh &mesh) { check(mlsgpu_hip_host_mesher_add(h, chunkId, &mesh)); }
    std::size_t write(const Namer &namer, const std::vector<std::string> &comments = std::vector<std::string>())
    {
        std::uint32_t chunks = 0;
        check(mlsgpu_hip_host_mesher_finalize(h, &chunks));
        std::vector<const char *> cstr;
        for (const std::string &c : comments)
            cstr.push_back(c.c_str());
        for (std::uint32_t i = 0; i < chunks; i++)
        {
            std::uint64_t id, nv, nt;
            const float *v;
            const std::uint32_t *t;
            check(mlsgpu_hip_host_mesher_chunk(h, i, &id, &nv, &nt, &v, &t));
            check(mlsgpu_hip_write_ply(namer(id).c_str(), v, nv, t, nt, cstr.empty() ? NULL : cstr.data(),
                                       (std::uint32_t) cstr.size()));
        }
        return chunks;
    }
    void getStatistics(std::uint64_t out[8]) const { check(mlsgpu_hip_host_mesher_stats(h, out)); }
};

/**
 * SplatSet::FileSet (src/splat_set.h:383-700): several PLY files read as one splat sequence; load() is the bounded-memory
 * route into HBM (reader threads + pinned quarters + H2D overlap).
 */
class FileSet
{
    mlsgpu_fileset *h;
    FileSet(const FileSet &);
    FileSet &operator=(const FileSet &);
public:
    FileSet(float smooth, float maxRadius) : h(NULL) { check(mlsgpu_hip_fileset_create(smooth, maxRadius, &h)); }
    ~FileSet() { mlsgpu_hip_fileset_destroy(h); }
    void addFile(const std::string &path) { check(mlsgpu_hip_fileset_add_file(h, path.c_str())); }
    void setBufferSize(std::uint64_t bytes) { check(mlsgpu_hip_fileset_set_buffer_size(h, bytes)); }
    std::uint64_t maxSplats() const { return mlsgpu_hip_fileset_num_splats(h); }
    mlsgpu_fileset *get() const { return h; }
    /// FastBlobSet::getBoundingGrid for a set that need not fit the device: one pass over the files
    mlsgpu_grid boundingGrid(const Context &ctx, float spacing, std::uint32_t bucketSize, std::uint64_t chunkSplats,
                             unsigned readerThreads = 0)
    {
        mlsgpu_grid g;
        check(mlsgpu_hip_fileset_bounding_grid(h, ctx.get(), spacing, bucketSize, chunkSplats, readerThreads, &g));
        return g;
    }
    void read(std::uint64_t first, std::uint64_t count, Splat *out) { check(mlsgpu_hip_fileset_read(h, first, count, out)); }
    void load(const Context &ctx, const Buffer<Splat> &out, std::uint64_t first, std::uint64_t count, unsigned readerThreads = 0)
    {
        check(mlsgpu_hip_fileset_load(h, ctx.get(), first, count, out.get(), readerThreads));
    }
};

/**
 * CopyGroup + one DeviceWorkerGroup per GPU inside the library (mlsgpu_hip_farm_*; src/workers.h:214-438,
 * src/mlsgpu_core.cpp:704-741).  Ship-outs go to a DeviceMesher (appended in HBM, by peer copy from other GPUs) or, with
 * setHostOutput, through the pinned circular buffer to an OOCMesher on the farm's mesher thread (the reference's route,
 * src/workers.h:488-509).
 */
class BucketFarm
{
    mlsgpu_farm *h;
    BucketFarm(const BucketFarm &);
    BucketFarm &operator=(const BucketFarm &);
public:
    BucketFarm(const std::vector<std::int32_t> &devices, const mlsgpu_worker_config &worker, unsigned workersPerDevice,
               unsigned spare, DeviceMesher *deviceSink = NULL) : h(NULL)
    {
        mlsgpu_farm_config cfg;
        std::memset(&cfg, 0, sizeof(cfg));
        cfg.numDevices = (std::uint32_t) devices.size();
        cfg.devices = devices.data();
        cfg.workersPerDevice = workersPerDevice;
        cfg.spare = spare;
        cfg.worker = worker;
        check(mlsgpu_hip_farm_create(&cfg, deviceSink ? &mlsgpu_hip_mesher_farm_output : NULL,
                                     deviceSink ? deviceSink->get() : NULL, &h));
    }
    ~BucketFarm() { mlsgpu_hip_farm_destroy(h); }
    mlsgpu_farm *get() const { return h; }
    void setHostOutput(std::uint64_t ringBytes, OOCMesher &mesher)
    {
        check(mlsgpu_hip_farm_set_host_output(h, ringBytes, &mlsgpu_hip_host_mesher_farm_output, mesher.get()));
        // a welder that has not been placed joins the ring's NUMA node (ignored once its threads exist)
        std::int32_t where[100];
        if (mesher.node() < 0 && mlsgpu_hip_farm_placement(h, where) == MLSGPU_OK && where[1] >= 0)
            (void) mlsgpu_hip_host_mesher_set_node(mesher.get(), where[1]);
    }
    Splat *acquire(std::uint64_t numSplats)                                 // CopyGroup::get
    {
        Splat *p = NULL;
        check(mlsgpu_hip_farm_acquire(h, numSplats, &p));
        return p;
    }
    void push(std::uint64_t numSplats, const BucketGrid &grid, std::uint64_t chunkId)     // CopyGroup::push
    {
        check(mlsgpu_hip_farm_push(h, numSplats, grid.low, grid.numVertices, chunkId));
    }
    void submitDevice(int device, const Buffer<Splat> &cloud, const mlsgpu_bucket &bin, const mlsgpu_grid &fullGrid,
                      std::uint64_t chunkId)
    {
        BucketGrid g;
        for (int i = 0; i < 3; i++)
        {
            g.low[i] = bin.extents[2 * i] - fullGrid.extents[2 * i];
            g.numVertices[i] = (std::uint32_t) (bin.extents[2 * i + 1] - bin.extents[2 * i] + 1);
        }
        // a resident cloud: only enqueued -- the bucketer orders the reuse of the bin's id list behind the gather on the GPU
        // (mlsgpu_bucket::consumed), so the leaves of a level reach the farm back to back and its workers batch them
        if (bin.consumed != NULL)
            check(mlsgpu_hip_farm_submit_device_async(h, device, cloud.get(), bin.dIds, bin.numSplats, &fullGrid, g.low,
                                                      g.numVertices, chunkId, bin.consumed));
        else
            check(mlsgpu_hip_farm_submit_device(h, device, cloud.get(), bin.dIds, bin.numSplats, &fullGrid, g.low, g.numVertices,
                                                chunkId));
    }
    /// the same for a bin of Bucket::bucketStream: its splats are in the batch that is resident during the callback
    void submitDevice(int device, const mlsgpu_bucket &bin, const mlsgpu_grid &fullGrid, std::uint64_t chunkId)
    {
        BucketGrid g;
        for (int i = 0; i < 3; i++)
        {
            g.low[i] = bin.extents[2 * i] - fullGrid.extents[2 * i];
            g.numVertices[i] = (std::uint32_t) (bin.extents[2 * i + 1] - bin.extents[2 * i] + 1);
        }
        check(mlsgpu_hip_farm_submit_device(h, device, bin.dSplats, bin.dIds, bin.numSplats, &fullGrid, g.low, g.numVertices,
                                            chunkId));
    }
    void finish() { check(mlsgpu_hip_farm_finish(h)); }
};

/**
 * Bucket::bucket (src/bucket.h:116-180) for a cloud that is resident on the device, and the device half of
 * BucketLoader (src/bucket_loader.cpp:77-102).  The processor receives the bucket's grid, recursion state and its
 * splat ids (device memory, ascending, valid during the call) where the reference's receives a splat subset.
 */
namespace Bucket
{

typedef mlsgpu_grid Grid;                   // src/grid.h: reference, spacing, per-axis [first, second) extents
typedef mlsgpu_bucket Bin;                  // extents, Recursion::chunk / depth, numSplats, dIds

/// Bucket::DensityError, src/bucket.h:52-65
class DensityError : public std::runtime_error
{
    std::uint64_t cellSplats;
public:
    explicit DensityError(std::uint64_t cellSplats)
        : std::runtime_error("Too many splats covering one cell"), cellSplats(cellSplats) {}
    std::uint64_t getCellSplats() const { return cellSplats; }
};

typedef std::function<void(const Bin &)> Processor;

namespace detail
{
struct Thunk
{
    const Processor *process;
    std::exception_ptr error;
    static int call(void *user, mlsgpu_ctx *, const mlsgpu_bucket *b)
    {
        Thunk *self = static_cast<Thunk *>(user);
        try
        {
            (*self->process)(*b);
            return 0;
        }
        catch (...)
        {
            self->error = std::current_exception();
            return 1;
        }
    }
};
} // namespace detail

inline void bucket(const Context &ctx, const Buffer<Splat> &splats, std::uint64_t numSplats, const Grid &region,
                   std::uint64_t maxSplats, std::uint32_t maxCells, std::uint32_t chunkCells, std::uint32_t microCells,
                   std::uint64_t maxSplit, const Processor &process)
{
    mlsgpu_bucket_params p;
    p.maxSplats = maxSplats;
    p.maxCells = maxCells;
    p.chunkCells = chunkCells;
    p.microCells = microCells;
    p.maxSplit = maxSplit;
    detail::Thunk thunk{&process, std::exception_ptr()};
    std::uint64_t cellSplats = 0;
    const int rc = mlsgpu_hip_bucket(ctx.get(), splats.get(), numSplats, &region, &p, &detail::Thunk::call, &thunk, &cellSplats);
    if (thunk.error)
        std::rethrow_exception(thunk.error);
    if (rc == MLSGPU_ERR_DENSITY)
        throw DensityError(cellSplats);
    check(rc);
}

/// Bucket::bucket over a FileSet that need NOT fit the device (mlsgpu_hip_bucket_stream): the files are streamed through a
/// chunk buffer, once to count and once per batch of top-level regions that fit `budgetSplats`; bin.dSplats is the batch
/// the ids index, valid during the call.  Same bins as bucket() makes of the set resident.
inline void bucketStream(const Context &ctx, FileSet &files, const Grid &region, std::uint64_t maxSplats, std::uint32_t maxCells,
                         std::uint32_t chunkCells, std::uint32_t microCells, std::uint64_t maxSplit, std::uint64_t budgetSplats,
                         std::uint64_t chunkSplats, unsigned readerThreads, const Processor &process, std::uint64_t stats[4] = NULL)
{
    mlsgpu_bucket_params p;
    p.maxSplats = maxSplats;
    p.maxCells = maxCells;
    p.chunkCells = chunkCells;
    p.microCells = microCells;
    p.maxSplit = maxSplit;
    detail::Thunk thunk{&process, std::exception_ptr()};
    std::uint64_t cellSplats = 0;
    const int rc = mlsgpu_hip_bucket_stream(ctx.get(), files.get(), &region, &p, budgetSplats, chunkSplats, readerThreads,
                                            &detail::Thunk::call, &thunk, &cellSplats, stats);
    if (thunk.error)
        std::rethrow_exception(thunk.error);
    if (rc == MLSGPU_ERR_DENSITY)
        throw DensityError(cellSplats);
    check(rc);
}

/// Gathers a bin's splats into `out` in the full grid's vertex coordinates and returns the sub-grid the worker needs
/// (BucketLoader::operator(), src/bucket_loader.cpp:77-102).
inline BucketGrid load(const Context &ctx, const Buffer<Splat> &splats, const Bin &bin, const Grid &fullGrid,
                       const Buffer<Splat> &out)
{
    check(mlsgpu_hip_bucket_load(ctx.get(), splats.get(), bin.dIds, bin.numSplats, &fullGrid, out.get()));
    BucketGrid g;
    for (int i = 0; i < 3; i++)
    {
        g.low[i] = bin.extents[2 * i] - fullGrid.extents[2 * i];
        g.numVertices[i] = (std::uint32_t) (bin.extents[2 * i + 1] - bin.extents[2 * i] + 1);
    }
    return g;
}

} // namespace Bucket

} // namespace hip
} // namespace mlsgpu

#endif /* MLSGPU_AMD_HOST_HPP */
