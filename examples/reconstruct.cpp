/*
 * PLY files of splats in, PLY mesh out, everything between on the device(s): the shape of the reference's main pipeline
 * (src/mlsgpu_core.cpp:560-760: load -> bounding grid -> Bucket::bucket -> BucketLoader -> device workers -> mesher ->
 * FastPly::Writer) with this repository's pieces:
 *   SplatSet::FileSet    mlsgpu::hip::FileSet         (several files, reader threads, bounded pinned memory, H2D overlap)
 *   bounding grid        mlsgpu_hip_bounding_grid     (device reduction)
 *   Bucket::bucket       mlsgpu::hip::Bucket::bucket  (device)
 *   BucketLoader + CopyGroup + DeviceWorkerGroup      mlsgpu::hip::BucketFarm::submitDevice (device gather + transform
 *                        into a device item of the least-loaded GPU -- a peer copy when that is another GPU -- then four
 *                        worker threads per GPU: octree, MLS, marching, scale/bias)
 *   OOCMesher            --weld device: mlsgpu::hip::DeviceMesher (ship-outs appended in one GPU's HBM, weld / components /
 *                        prune there); --weld host: every ship-out read back through the pinned circular buffer and welded
 *                        by mlsgpu::hip::OOCMesher on the mesher thread (the reference's route)
 *
 * usage: reconstruct [--devices 0,1,...] [--weld device|host] [--check] [--fill-holes N] [--simplify N | --simplify-quadric N] [--repair [pinches]] [--split-edges F] [--collapse-edges F] [--flip-edges R] [--smooth N] [--deviation D] [--self-intersections] [--compact BITS] [--normals] [--tmp-dir DIR] [--buffer BYTES] <in.ply> [more.ply ...] <out.ply>
 *                    <spacing> [smooth=4] [levels=6] [subsampling=3] [prune=0.02] [maxSplats=2097152]
 * (defaults as src/mlsgpu_core.cpp:86-135: --fit-smooth 4, --levels 6, --subsampling 3, --fit-prune 0.02)
 * --check (device weld only): after the write, Manifold::isManifold on every output chunk where it lies, one line each.
 * --fill-holes N (device weld only, 3 <= N <= 1048576): directly after the weld, every boundary loop of at most N sides of every
 *   output chunk is capped by a fan to the mean of its vertices, where the chunk lies -- before --check, --simplify, --smooth
 *   and --normals; the loops on a seam between two chunks stay open; one line with the statistics.
 * --simplify N (device weld only, N > 0): before the write, every output chunk is vertex-clustered where it lies, in cells of
 *   N grid spacings counted from one cell below the bounding grid's low corner; one line with the statistics.
 * --simplify-quadric N (device weld only, N > 0, not with --simplify): the same clustering in the same place, with every
 *   cluster's vertex at the minimiser of its triangles' plane quadrics, which keeps the creases that the mean chamfers; one
 *   line with the statistics.
 * --repair, --repair pinches (device weld only): before the write, every output chunk is repaired where it lies: triangles
 *   with a repeated directed side are dropped and pinched vertices split (with `pinches`: every umbrella of a vertex becomes a
 *   vertex of its own), so that --check says `manifold yes` -- after --simplify, which can make a chunk non-manifold, and
 *   before --flip-edges, --smooth, --normals and --check; one line with the statistics.
 * --split-edges F (device weld only, F > 0 in grid spacings): before the write, the edges of every output chunk that are
 *   longer than F spacings are halved where the chunk lies, the longest side of a triangle first (at most 64 rounds, a chunk
 *   grows to at most 16 times its triangles): the refine step that gives the fans of --fill-holes and the cells of --simplify
 *   an even triangle size; with several chunks the seams stay as they are -- after --fill-holes, --simplify and --repair,
 *   before --collapse-edges, --flip-edges, --smooth, --deviation and --normals; one line with the statistics, the smallest
 *   triangle quality and the longest edge before and after.
 * --collapse-edges F (device weld only, F > 0 in grid spacings): before the write, the interior edges of every output chunk
 *   that are at most F spacings long are collapsed where the chunk lies (minCos 0.5, at most 64 rounds): a vertex and two
 *   triangles go per edge -- the needles that marching leaves where the surface passes close to a lattice vertex --, the
 *   vertices on a chunk's boundary stay, and so does the topology -- after --simplify and --repair, before --flip-edges,
 *   --smooth and --normals; one line with the statistics and the smallest triangle quality before and after.
 * --flip-edges R (device weld only, R > 0): before the write, every output chunk goes through at most R rounds of Delaunay edge
 *   flips where it lies (minGain 1e-6, minCos 0.5): connectivity only, the vertices and the edges on a chunk's boundary stay
 *   -- after --simplify and --repair, before --smooth; one line with the statistics and the smallest triangle quality before
 *   and after.
 * --smooth N (device weld only, N > 0): before the write, every output chunk gets N Taubin iterations (lambda 0.5, mu -0.53)
 *   where it lies, the vertices on a chunk's boundary held fixed -- after --simplify and --flip-edges when they are given; one line with the
 *   statistics.
 * --deviation D (device weld only, D > 0 in world units): the chunks are kept as the weld left them, and after the last of
 *   --fill-holes, --simplify, --repair, --split-edges, --collapse-edges, --flip-edges and --smooth two lines say how far the output lies from them: `moved`, the output's
 *   vertices against the kept surface, and `lost`, the kept vertices against the output's surface -- the points within and
 *   beyond D, the largest and the RMS distance, and the distances that 50 % and 90 % of the points within stay under, read
 *   off a histogram of 16 bins.  Without such a stage `moved` is all zeros.
 * --self-intersections (device weld only): after the last of those stages and before the write, the triangle pairs of every
 *   output chunk that certainly pass through each other are counted where the chunk lies (pairs across chunks are not looked
 *   for; touching and coplanar overlap are not reported): one line, `self-intersections pairs N triangles N chunks N first C A
 *   B` -- the lowest chunk that has a pair and its lowest pair -- or `first -`.  The output files are the same with and without.
 * --compact BITS (device weld only; BITS 32 or 8..24): every output chunk comes back as a compact blob -- encoded where it lies,
 *   one copy across the link, decoded on the host -- and the decoded arrays go to the same PLY writer.  One line, `compact bits B
 *   raw N blob N ratio R exceptions N step X Y Z` (bytes summed over the chunks, the largest quantisation step per axis).  With
 *   32 the files are byte-identical to those written without the flag; below, vertices move by at most half a step.
 * --normals (device weld only): every output chunk is written with its area-weighted vertex normals (nx ny nz after z),
 *   computed where the chunk lies -- after --simplify and --smooth when they are given; one line per chunk.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <limits>
#include <sstream>
#include <vector>

#include "../mlsgpu_amd/host/mlsgpu_hip.hpp"

using namespace mlsgpu::hip;

// the distance that `share` of the points within stay under: the upper edge of the histogram bin where their count is reached
static double quantileOf(const mlsgpu_deviation &d, double share)
{
    std::uint64_t seen = 0;
    for (int k = 0; k < 16; k++)
    {
        seen += d.histogram[k];
        if (d.within > 0 && (double) seen >= share * (double) d.within)
            return std::sqrt(d.limit2) * (k + 1) / 16.0;
    }
    return 0.0;
}

static void printDeviation(const char *name, const mlsgpu_deviation &d)
{
    const double meanSquare = d.within > 0 ? std::ldexp((double) d.sumQ, (int) d.scaleExponent - 30) / (double) d.within : 0.0;
    std::printf("deviation %s points %llu within %llu beyond %llu max %.9g rms %.9g p50 %.9g p90 %.9g\n", name,
                (unsigned long long) d.numPoints, (unsigned long long) d.within, (unsigned long long) d.beyond,
                std::sqrt(d.maxDistance2), std::sqrt(meanSquare), quantileOf(d, 0.5), quantileOf(d, 0.9));
}

static bool isPly(const std::string &a) { return a.size() > 4 && a.compare(a.size() - 4, 4, ".ply") == 0; }

int main(int argc, char **argv)
{
    std::vector<std::int32_t> devices(1, 0);
    bool hostWeld = false, checkTopology = false, writeNormals = false;
    std::uint64_t bufferBytes = 0, hbmSplats = 0;
    float simplifyCells = 0.0f;
    bool simplifyGiven = false, quadricGiven = false, smoothGiven = false, fillGiven = false, repairGiven = false;
    std::uint32_t repairFlags = 0;
    long smoothIterations = 0, fillEdges = 0, flipRounds = 0;
    bool flipGiven = false, collapseGiven = false, splitGiven = false;
    double collapseSpacings = 0.0, splitSpacings = 0.0;
    float deviationDistance = 0.0f;
    bool deviationGiven = false, intersectionsGiven = false;
    long compactBits = 0;
    std::string tmpDir;
    std::vector<std::string> plys, rest;
    for (int i = 1; i < argc; i++)
    {
        const std::string a = argv[i];
        if (a == "--devices" && i + 1 < argc)
        {
            devices.clear();
            std::istringstream ss(argv[++i]);
            std::string tok;
            while (std::getline(ss, tok, ','))
                devices.push_back(atoi(tok.c_str()));
        }
        else if (a == "--weld" && i + 1 < argc)
            hostWeld = std::string(argv[++i]) == "host";
        else if (a == "--check")
            checkTopology = true;
        else if (a == "--normals")
            writeNormals = true;
        else if (a == "--simplify" && i + 1 < argc)
        {
            simplifyCells = (float) atof(argv[++i]);
            simplifyGiven = true;
        }
        else if (a == "--simplify-quadric" && i + 1 < argc)
        {
            simplifyCells = (float) atof(argv[++i]);
            quadricGiven = true;
        }
        else if (a == "--smooth" && i + 1 < argc)
        {
            smoothIterations = atol(argv[++i]);
            smoothGiven = true;
        }
        else if (a == "--flip-edges" && i + 1 < argc)
        {
            flipRounds = atol(argv[++i]);
            flipGiven = true;
        }
        else if (a == "--split-edges" && i + 1 < argc)
        {
            splitSpacings = atof(argv[++i]);
            splitGiven = true;
        }
        else if (a == "--collapse-edges" && i + 1 < argc)
        {
            collapseSpacings = atof(argv[++i]);
            collapseGiven = true;
        }
        else if (a == "--fill-holes" && i + 1 < argc)
        {
            fillEdges = atol(argv[++i]);
            fillGiven = true;
        }
        else if (a == "--deviation" && i + 1 < argc)
        {
            deviationDistance = (float) atof(argv[++i]);
            deviationGiven = true;
        }
        else if (a == "--self-intersections")
            intersectionsGiven = true;
        else if (a == "--compact" && i + 1 < argc)
        {
            compactBits = atol(argv[++i]);
            if (compactBits != 32 && (compactBits < 8 || compactBits > 24))
            {
                std::cerr << "--compact takes 32 or 8..24\n";
                return 2;
            }
        }
        else if (a == "--repair")
        {
            repairGiven = true;
            if (i + 1 < argc && std::string(argv[i + 1]) == "pinches")
            {
                repairFlags = MLSGPU_REPAIR_SPLIT_PINCHES;
                i++;
            }
        }
        else if (a == "--buffer" && i + 1 < argc)
            bufferBytes = strtoull(argv[++i], NULL, 10);
        else if (a == "--tmp-dir" && i + 1 < argc)             // --weld host: the welder's blocks in temporary files there (src/mlsgpu_core.cpp --tmp-dir)
            tmpDir = argv[++i];
        else if (a == "--hbm-splats" && i + 1 < argc)       // the cloud does not fit the device: stream it, this many at a time
            hbmSplats = strtoull(argv[++i], NULL, 10);
        else if (rest.empty() && isPly(a))
            plys.push_back(a);
        else
            rest.push_back(a);
    }
    if (plys.size() < 2 || rest.empty() || devices.empty())
    {
        std::cerr << "usage: reconstruct [--devices 0,1] [--weld device|host] [--check] [--fill-holes N] [--simplify N | --simplify-quadric N] [--repair [pinches]] [--split-edges F] [--collapse-edges F] [--flip-edges R] [--smooth N] [--deviation D] [--self-intersections] [--compact BITS] [--normals] [--tmp-dir DIR] [--buffer BYTES] [--hbm-splats N] in.ply [more.ply ...] out.ply "
                     "spacing [smooth] [levels] [subsampling] [prune] [maxSplats]\n";
        return 2;
    }
    if (simplifyGiven && quadricGiven)
    {
        std::cerr << "--simplify and --simplify-quadric exclude each other: a chunk is clustered once\n";
        return 2;
    }
    if (quadricGiven && !(simplifyCells > 0.0f && simplifyCells <= std::numeric_limits<float>::max()))
    {
        std::cerr << "--simplify-quadric takes a number of grid spacings > 0\n";
        return 2;
    }
    if (quadricGiven && hostWeld)
    {
        std::cerr << "--simplify-quadric needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (simplifyGiven && !(simplifyCells > 0.0f && simplifyCells <= std::numeric_limits<float>::max()))
    {
        std::cerr << "--simplify takes a number of grid spacings > 0\n";
        return 2;
    }
    if (simplifyGiven && hostWeld)
    {
        std::cerr << "--simplify needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (smoothGiven && !(smoothIterations > 0 && smoothIterations <= 1000000))
    {
        std::cerr << "--smooth takes a number of iterations > 0\n";
        return 2;
    }
    if (smoothGiven && hostWeld)
    {
        std::cerr << "--smooth needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (flipGiven && !(flipRounds > 0 && flipRounds <= 1000000))
    {
        std::cerr << "--flip-edges takes a number of rounds > 0\n";
        return 2;
    }
    if (flipGiven && hostWeld)
    {
        std::cerr << "--flip-edges needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (splitGiven && !(splitSpacings > 0.0 && splitSpacings <= std::numeric_limits<float>::max()))
    {
        std::cerr << "--split-edges takes a number of grid spacings > 0\n";
        return 2;
    }
    if (splitGiven && hostWeld)
    {
        std::cerr << "--split-edges needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (collapseGiven && !(collapseSpacings > 0.0 && collapseSpacings <= std::numeric_limits<float>::max()))
    {
        std::cerr << "--collapse-edges takes a number of grid spacings > 0\n";
        return 2;
    }
    if (collapseGiven && hostWeld)
    {
        std::cerr << "--collapse-edges needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (fillGiven && !(fillEdges >= 3 && fillEdges <= (long) MLSGPU_FILL_MAX_EDGES))
    {
        std::cerr << "--fill-holes takes the longest loop to fill, 3 to 1048576 sides\n";
        return 2;
    }
    if (fillGiven && hostWeld)
    {
        std::cerr << "--fill-holes needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (deviationGiven && !(deviationDistance > 0.0f && deviationDistance <= std::numeric_limits<float>::max()))
    {
        std::cerr << "--deviation takes a search distance > 0\n";
        return 2;
    }
    if (deviationGiven && hostWeld)
    {
        std::cerr << "--deviation needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (intersectionsGiven && hostWeld)
    {
        std::cerr << "--self-intersections needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (compactBits != 0 && (hostWeld || writeNormals))
    {
        std::cerr << (hostWeld ? "--compact needs --weld device: the host welder's output is not on the device\n"
                               : "--compact carries no normals: not with --normals\n");
        return 2;
    }
    if (repairGiven && hostWeld)
    {
        std::cerr << "--repair needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    if (writeNormals && hostWeld)
    {
        std::cerr << "--normals needs --weld device: the host welder's output is not on the device\n";
        return 2;
    }
    const std::string outName = plys.back();
    plys.pop_back();
    const float spacing = (float) atof(rest[0].c_str());
    const float smooth = rest.size() > 1 ? (float) atof(rest[1].c_str()) : 4.0f;
    const unsigned levels = rest.size() > 2 ? (unsigned) atoi(rest[2].c_str()) : 6;
    const unsigned subsampling = rest.size() > 3 ? (unsigned) atoi(rest[3].c_str()) : 3;
    const double prune = rest.size() > 4 ? atof(rest[4].c_str()) : 0.02;
    const std::uint64_t maxSplats = rest.size() > 5 ? strtoull(rest[5].c_str(), NULL, 10) : 2097152;
    const std::uint32_t maxCells = (1u << (levels + subsampling - 1)) - 1;        // src/mlsgpu_core.cpp:672-673
    const std::uint32_t microCells = std::min<std::uint32_t>(63, maxCells);          // --leaf-cells 63, :113,674
    try
    {
        FileSet files(smooth, std::numeric_limits<float>::infinity());
        for (const std::string &p : plys)
            files.addFile(p);
        if (bufferBytes)
            files.setBufferSize(bufferBytes);
        const std::uint64_t numSplats = files.maxSplats();
        if (numSplats == 0)
        {
            std::cerr << "no splats\n";
            return 1;
        }
        const int home = devices[0];                            // the cloud (and the device sink) live on the first GPU
        Context ctx(home);
        const bool streamed = hbmSplats != 0;                   // the set is larger than what may be resident at once
        const std::uint64_t chunkSplats = streamed ? std::max<std::uint64_t>(hbmSplats / 4, 1) : 0;
        Buffer<Splat> cloud(ctx, streamed ? 1 : numSplats);
        Bucket::Grid grid;
        if (streamed)
            grid = files.boundingGrid(ctx, spacing, microCells, chunkSplats);      // one pass over the files
        else
        {
            // files -> HBM: reader threads decode into pinned quarters while earlier chunks travel; no host copy of the cloud
            files.load(ctx, cloud, 0, numSplats);
            check(mlsgpu_hip_bounding_grid(ctx.get(), cloud.get(), numSplats, spacing, microCells, &grid));
        }

        mlsgpu_worker_config cfg;
        std::memset(&cfg, 0, sizeof(cfg));
        cfg.maxBucketSplats = maxSplats;
        cfg.maxCells = maxCells;
        cfg.levels = levels;
        cfg.subsampling = subsampling;
        cfg.boundaryLimit = 1.0f;
        cfg.shape = MLSGPU_SHAPE_SPHERE;
        cfg.gridSpacing = spacing;                             // ScaleBiasFilter: vertex * spacing + grid.getVertex(0,0,0)
        for (int i = 0; i < 3; i++)
            cfg.gridOrigin[i] = grid.reference[i] + spacing * (float) grid.extents[2 * i];

        DeviceMesher deviceMesher(ctx);
        deviceMesher.setPruneThreshold(prune);
        OOCMesher hostMesher;
        hostMesher.setPruneThreshold(prune);
        if (!tmpDir.empty())
            hostMesher.setTmpDir(tmpDir, 0);
        std::size_t bins = 0, written = 0;
        std::uint64_t st[8];
        mlsgpu_simplify_stats simplified = mlsgpu_simplify_stats();
        mlsgpu_simplify_quadric_stats placed = mlsgpu_simplify_quadric_stats();
        float simplifyCell = 0.0f, simplifyOrigin[3] = {0.0f, 0.0f, 0.0f};
        mlsgpu_smooth_stats smoothed = mlsgpu_smooth_stats();
        std::size_t smoothedChunks = 0;
        mlsgpu_fill_stats filled = mlsgpu_fill_stats();
        std::size_t filledChunks = 0;
        mlsgpu_repair_stats repaired = mlsgpu_repair_stats();
        std::size_t repairedChunks = 0;
        mlsgpu_collapse_stats collapsed = mlsgpu_collapse_stats();
        std::size_t collapsedChunks = 0;
        mlsgpu_split_stats split = mlsgpu_split_stats();
        std::size_t splitChunks = 0;
        mlsgpu_flip_stats flipped = mlsgpu_flip_stats();
        std::size_t flippedChunks = 0;
        std::pair<mlsgpu_deviation, mlsgpu_deviation> deviated;
        mlsgpu_self_intersections crossed = mlsgpu_self_intersections();
        mlsgpu_compact_stats compacted = mlsgpu_compact_stats();
        std::uint64_t compactRaw = 0;
        {
            BucketFarm farm(devices, cfg, 4 /* --device-threads */, 1, hostWeld ? NULL : &deviceMesher);
            if (hostWeld)
                farm.setHostOutput(std::uint64_t(512) << 20 /* --mem-mesh */, hostMesher);
            if (streamed)
                // out of core: the files streamed through a chunk buffer, a batch of top-level regions resident at a time
                Bucket::bucketStream(ctx, files, grid, maxSplats, maxCells, 0, microCells, std::uint64_t(1) << 30, hbmSplats,
                                     chunkSplats, 0, [&](const Bucket::Bin &bin)
                {
                    farm.submitDevice(home, bin, grid, 0);
                    bins++;
                });
            else
                Bucket::bucket(ctx, cloud, numSplats, grid, maxSplats, maxCells, 0, microCells, std::uint64_t(1) << 30,
                               [&](const Bucket::Bin &bin)
                {
                    farm.submitDevice(home, cloud, bin, grid, 0);
                    bins++;
                });
            farm.finish();
        }
        const std::vector<std::string> comments(1, "mlsgpu-hip example: reconstruct");
        if (hostWeld)
        {
            written = hostMesher.write([&](std::uint64_t) { return outName; }, comments);
            hostMesher.getStatistics(st);
        }
        else
        {
            const std::size_t chunks = deviceMesher.finalize();
            if (deviationGiven)
                deviceMesher.keepReference();       // directly behind the weld: what every later stage is measured against
            if (fillGiven)
            {
                filled = deviceMesher.fillHoles((std::uint32_t) fillEdges);
                filledChunks = chunks;
            }
            if (simplifyGiven || quadricGiven)
            {
                simplifyCell = simplifyCells * spacing;
                for (int i = 0; i < 3; i++)
                    simplifyOrigin[i] = cfg.gridOrigin[i] - simplifyCell;
                if (quadricGiven)
                    placed = deviceMesher.simplifyQuadric(simplifyOrigin, simplifyCell);
                else
                    simplified = deviceMesher.simplify(simplifyOrigin, simplifyCell);
            }
            if (repairGiven)
            {
                repaired = deviceMesher.repair(repairFlags);
                repairedChunks = chunks;
            }
            if (splitGiven)
            {
                split = deviceMesher.splitEdges(64, splitSpacings * spacing, 16);
                splitChunks = chunks;
            }
            if (collapseGiven)
            {
                collapsed = deviceMesher.collapseEdges(64, collapseSpacings * spacing, 0.5);
                collapsedChunks = chunks;
            }
            if (flipGiven)
            {
                flipped = deviceMesher.flipEdges((std::uint32_t) flipRounds, 1e-6, 0.5);
                flippedChunks = chunks;
            }
            if (smoothGiven)
            {
                smoothed = deviceMesher.smooth((std::uint32_t) smoothIterations, 0.5f, -0.53f, MLSGPU_SMOOTH_BOUNDARY_FIXED);
                smoothedChunks = chunks;
            }
            if (deviationGiven)
                deviated = deviceMesher.deviation(deviationDistance);
            if (intersectionsGiven)
                crossed = deviceMesher.selfIntersections();
            if (compactBits != 0)
            {
                // encode -> copy -> decode, then the writer of host arrays: the same file as straight from HBM
                std::vector<std::uint32_t> blob, triangles;
                std::vector<float> vertices;
                const char *const comment = comments[0].c_str();
                for (std::uint32_t i = 0; i < chunks; i++)
                {
                    const mlsgpu_compact_stats one = deviceMesher.chunkCompact(i, (std::uint32_t) compactBits, blob);
                    compactDecode(blob.data(), one.blobBytes, vertices, triangles);
                    check(mlsgpu_hip_write_ply(outName.c_str(), vertices.data(), one.numVertices, triangles.data(), one.numTriangles,
                                               &comment, 1));
                    compactRaw += 12 * (one.numVertices + one.numTriangles);
                    compacted.blobBytes += one.blobBytes;
                    compacted.exceptions += one.exceptions;
                    for (int a = 0; a < 3; a++)
                        compacted.step[a] = std::max(compacted.step[a], one.step[a]);
                }
                written = chunks;
            }
            else
                written = deviceMesher.writeChunks(chunks, [&](std::uint64_t) { return outName; }, comments, writeNormals);
            deviceMesher.getStatistics(st);
        }
        std::printf("files in %zu splats %llu grid %d..%d %d..%d %d..%d bins %zu devices %zu weld %s files %zu vertices %llu "
                    "triangles %llu components %llu kept %llu\n",
                    plys.size(), (unsigned long long) numSplats, grid.extents[0], grid.extents[1], grid.extents[2],
                    grid.extents[3], grid.extents[4], grid.extents[5], bins, devices.size(), hostWeld ? "host" : "device",
                    written, (unsigned long long) st[4], (unsigned long long) st[5], (unsigned long long) st[2],
                    (unsigned long long) st[3]);
        if (fillGiven)
            std::printf("fill-holes chunks %zu boundary-edges %llu loops %llu filled %llu long %llu pinned %llu irregular-edges %llu "
                        "vertices %llu -> %llu triangles %llu -> %llu\n",
                        filledChunks, (unsigned long long) filled.boundaryEdges, (unsigned long long) filled.loops,
                        (unsigned long long) filled.filledLoops, (unsigned long long) filled.longLoops,
                        (unsigned long long) filled.pinnedLoops, (unsigned long long) filled.irregularEdges,
                        (unsigned long long) filled.numVertices, (unsigned long long) filled.outVertices,
                        (unsigned long long) filled.numTriangles, (unsigned long long) filled.outTriangles);
        if (simplifyGiven)
            std::printf("simplify cell %.9g origin %.9g %.9g %.9g vertices %llu -> %llu triangles %llu -> %llu collapsed %llu "
                        "duplicate %llu\n",
                        simplifyCell, simplifyOrigin[0], simplifyOrigin[1], simplifyOrigin[2],
                        (unsigned long long) simplified.inVertices, (unsigned long long) simplified.outVertices,
                        (unsigned long long) simplified.inTriangles, (unsigned long long) simplified.outTriangles,
                        (unsigned long long) simplified.collapsedTriangles, (unsigned long long) simplified.duplicateTriangles);
        if (quadricGiven)
            std::printf("simplify-quadric cell %.9g origin %.9g %.9g %.9g vertices %llu -> %llu triangles %llu -> %llu collapsed %llu "
                        "duplicate %llu solved %llu flat %llu escaped %llu scale-exponent %lld\n",
                        simplifyCell, simplifyOrigin[0], simplifyOrigin[1], simplifyOrigin[2],
                        (unsigned long long) placed.inVertices, (unsigned long long) placed.outVertices,
                        (unsigned long long) placed.inTriangles, (unsigned long long) placed.outTriangles,
                        (unsigned long long) placed.collapsedTriangles, (unsigned long long) placed.duplicateTriangles,
                        (unsigned long long) placed.solvedVertices, (unsigned long long) placed.flatVertices,
                        (unsigned long long) placed.escapedVertices, (long long) placed.scaleExponent);
        if (repairGiven)
            std::printf("repair chunks %zu out-of-range %llu degenerate %llu repeated-sides %llu dropped %llu unused %llu split %llu "
                        "vertices %llu -> %llu triangles %llu -> %llu\n",
                        repairedChunks, (unsigned long long) repaired.outOfRangeTriangles, (unsigned long long) repaired.degenerateTriangles,
                        (unsigned long long) repaired.repeatedSides, (unsigned long long) repaired.droppedTriangles,
                        (unsigned long long) repaired.unusedVertices, (unsigned long long) repaired.splitVertices,
                        (unsigned long long) repaired.numVertices, (unsigned long long) repaired.outVertices,
                        (unsigned long long) repaired.numTriangles, (unsigned long long) repaired.outTriangles);
        if (splitGiven)
            std::printf("split-edges chunks %zu interior-edges %llu boundary-edges %llu rounds %llu splits %llu boundary %llu "
                        "long %llu -> %llu blocked %llu limited %llu vertices %llu -> %llu triangles %llu -> %llu "
                        "min-quality %.9g -> %.9g max-length %.9g -> %.9g\n",
                        splitChunks, (unsigned long long) split.interiorEdges, (unsigned long long) split.boundaryEdges,
                        (unsigned long long) split.rounds, (unsigned long long) split.splits, (unsigned long long) split.boundarySplits,
                        (unsigned long long) split.longBefore, (unsigned long long) split.longAfter,
                        (unsigned long long) split.blockedAfter, (unsigned long long) split.limited,
                        (unsigned long long) split.numVertices, (unsigned long long) split.outVertices,
                        (unsigned long long) split.numTriangles, (unsigned long long) split.outTriangles, split.minQualityBefore,
                        split.minQualityAfter, std::sqrt(split.maxLengthSqBefore), std::sqrt(split.maxLengthSqAfter));
        if (collapseGiven)
            std::printf("collapse-edges chunks %zu interior-edges %llu fixed %llu rounds %llu collapses %llu short %llu -> %llu "
                        "blocked %llu vertices %llu -> %llu triangles %llu -> %llu min-quality %.9g -> %.9g\n",
                        collapsedChunks, (unsigned long long) collapsed.interiorEdges, (unsigned long long) collapsed.fixedVertices,
                        (unsigned long long) collapsed.rounds, (unsigned long long) collapsed.collapses,
                        (unsigned long long) collapsed.shortBefore, (unsigned long long) collapsed.shortAfter,
                        (unsigned long long) collapsed.blockedAfter, (unsigned long long) collapsed.numVertices,
                        (unsigned long long) collapsed.outVertices, (unsigned long long) collapsed.numTriangles,
                        (unsigned long long) collapsed.outTriangles, collapsed.minQualityBefore, collapsed.minQualityAfter);
        if (flipGiven)
            std::printf("flip-edges chunks %zu interior-edges %llu rounds %llu flips %llu non-delaunay %llu -> %llu blocked %llu "
                        "min-quality %.9g -> %.9g\n",
                        flippedChunks, (unsigned long long) flipped.interiorEdges, (unsigned long long) flipped.rounds,
                        (unsigned long long) flipped.flips, (unsigned long long) flipped.nonDelaunayBefore,
                        (unsigned long long) flipped.nonDelaunayAfter, (unsigned long long) flipped.blockedAfter,
                        flipped.minQualityBefore, flipped.minQualityAfter);
        if (smoothGiven)
            std::printf("smooth chunks %zu vertices %llu edges %llu boundary-vertices %llu isolated %llu passes %llu max-move %.9g\n",
                        smoothedChunks, (unsigned long long) smoothed.numVertices, (unsigned long long) smoothed.numEdges,
                        (unsigned long long) smoothed.boundaryVertices, (unsigned long long) smoothed.isolatedVertices,
                        (unsigned long long) smoothed.passes, smoothed.maxMove);
        if (deviationGiven)
        {
            printDeviation("moved", deviated.first);
            printDeviation("lost", deviated.second);
        }
        if (intersectionsGiven)
        {
            std::printf("self-intersections pairs %llu triangles %llu chunks %llu first", (unsigned long long) crossed.crossingPairs,
                        (unsigned long long) crossed.crossingTriangles, (unsigned long long) crossed.crossingChunks);
            if (crossed.crossingPairs > 0)
                std::printf(" %llu %llu %llu\n", (unsigned long long) crossed.lowestChunk, (unsigned long long) crossed.lowestA,
                            (unsigned long long) crossed.lowestB);
            else
                std::printf(" -\n");
        }
        if (compactBits != 0)
            std::printf("compact bits %ld raw %llu blob %llu ratio %.4f exceptions %llu step %.9g %.9g %.9g\n", compactBits,
                        (unsigned long long) compactRaw, (unsigned long long) compacted.blobBytes,
                        compactRaw ? (double) compacted.blobBytes / (double) compactRaw : 0.0, (unsigned long long) compacted.exceptions,
                        compacted.step[0], compacted.step[1], compacted.step[2]);
        if (writeNormals)
            for (std::uint32_t i = 0; i < written; i++)
            {
                std::uint64_t id = 0;
                check(mlsgpu_hip_mesher_chunk(deviceMesher.get(), i, &id, NULL, NULL, NULL, NULL));
                const mlsgpu_normals_stats n = deviceMesher.normals(i);        // what the writer computed, served again
                std::printf("normals chunk %llu vertices %llu zero %llu out-of-range %llu non-finite %llu exponent %lld\n",
                            (unsigned long long) id, (unsigned long long) n.numVertices, (unsigned long long) n.zeroNormals,
                            (unsigned long long) n.outOfRangeTriangles, (unsigned long long) n.nonFiniteTriangles,
                            (long long) n.scaleExponent);
            }
        if (checkTopology && !hostWeld)
            for (std::uint32_t i = 0; i < written; i++)
            {
                std::uint64_t id = 0;
                check(mlsgpu_hip_mesher_chunk(deviceMesher.get(), i, &id, NULL, NULL, NULL, NULL));
                const mlsgpu_topology t = deviceMesher.topology(i);
                const std::string why = Manifold::reason(t);
                std::printf("topology chunk %llu manifold %s components %llu boundaries %llu euler %lld boundary-edges %llu%s%s\n",
                            (unsigned long long) id, t.manifold ? "yes" : "no", (unsigned long long) t.numComponents,
                            (unsigned long long) t.numBoundaries, (long long) t.eulerCharacteristic,
                            (unsigned long long) t.boundaryEdges, why.empty() ? "" : " ", why.c_str());
            }
    }
    catch (std::exception &e)
    {
        std::cerr << "error: " << e.what() << "\n";
        return 1;
    }
    return 0;
}
