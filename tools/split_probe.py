#!/usr/bin/env python3
"""The long-edge split of chunk 0 of a finalized device sink, as the weld left it and after fill_holes, timed per kernel (HIP
events around every launch, the best of five calls) at several edge limits F (in grid spacings): per-kernel totals and launches
of a run to convergence, one classification alone (maxRounds 0) next to the collapse's on the same chunk, rounds, splits and
the mesh's size behind every round, the two quality histograms, how far the result lies from the input (the deviation report
both ways: rounding level, the surface is the input's), and the flips behind the split against the flips alone.
split_probe.py [cfg2|cfg3] [shells|uniform] [fill edges=64] [notes.md]"""
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.flip_probe import best_of  # noqa: E402

KERNELS = ("check", "work", "quality", "edges", "sort", "classify", "rewrite", "rows")
CLASSIFICATION = {"split": ("edges", "sort", "classify"), "collapse": ("records", "sort", "segments", "fixed", "classify")}
LIMITS = (1.5, 1.2, 0.9)
MAX_ROUNDS, MIN_COS, MIN_GAIN = 64, 0.5, 1e-6


def probe(ctx, m, b, chunk):
    """Split of one chunk where it lies, into buffers of its own, at every limit; flips behind the middle one."""
    from mlsgpu_amd.split_stats import SplitStats
    V, T = chunk["num_vertices"], chunk["num_triangles"]
    dv = m.DeviceBuffer(ctx, nbytes=12 * V, borrow=chunk["d_vertices"])
    dt = m.DeviceBuffer(ctx, nbytes=12 * T, borrow=chunk["d_triangles"])
    flipped = m.DeviceBuffer(ctx, nbytes=12 * T)
    out = {"vertices": V, "triangles": T, "limits": {}}
    entry = b.lib().mlsgpu_hip_mesh_split_edges

    def sizes(rounds, limit):
        st = SplitStats()
        rc = entry(ctx.h, dv.ptr, V, dt.ptr, T, rounds, limit, 0, None, None, 0, None, 0, None, C.byref(st))
        if rc != b._LENGTH:     # MLSGPU_ERR_LENGTH is the answer to the question
            b.check(rc)
        return st.as_dict()

    def split(rounds, limit, ov, cap_v, ot, cap_t):
        def call():
            st = SplitStats()
            b.check(entry(ctx.h, dv.ptr, V, dt.ptr, T, rounds, limit, 0, None, ov.ptr, cap_v, ot.ptr, cap_t, None, C.byref(st)))
            return st.as_dict()
        return call

    def collapse_report():
        st = b.CollapseStats()
        rc = b.lib().mlsgpu_hip_mesh_collapse_edges(ctx.h, dv.ptr, V, dt.ptr, T, 0, 0.2, MIN_COS, None, 0, None, 0, None, C.byref(st))
        if rc != b._LENGTH:
            b.check(rc)
        return st.as_dict()

    def flips(vertices, num_vertices, triangles, num_triangles, target, rounds):
        def call():
            st = b.FlipStats()
            b.check(b.lib().mlsgpu_hip_mesh_flip_edges(ctx.h, vertices.ptr, num_vertices, triangles.ptr, num_triangles, rounds, MIN_GAIN,
                                                       MIN_COS, target.ptr, C.byref(st)))
            return st.as_dict()
        return call

    def deviation(points, num_points, vertices, num_vertices, triangles, num_triangles, limit):
        r = b.mesh_deviation(ctx, points, vertices, triangles, limit, want_distances=False, want_nearest=False, num_points=num_points,
                             num_vertices=num_vertices, num_triangles=num_triangles)[2]
        return {"max": math.sqrt(r["maxDistance2"]), "rms": math.sqrt(r["meanSquare"]), "beyond": r["beyond"]}

    once = {"split": best_of(ctx, "kernel.split.", "split.scratch.bytes", lambda: sizes(0, LIMITS[1])),
            "collapse": best_of(ctx, "kernel.collapse.", "collapse.scratch.bytes", collapse_report)}
    out["classification"] = dict((k, {"ms": round(sum(r["stats"].get(n, 0.0) for n in CLASSIFICATION[k]), 4),
                                      "stats": dict((n, r["stats"].get(n, 0.0)) for n in CLASSIFICATION[k])}) for k, r in once.items())
    alone = best_of(ctx, "kernel.flip.", "flip.scratch.bytes", flips(dv, V, dt, T, flipped, MAX_ROUNDS))
    out["flips_alone"] = {"kernels_ms": alone["kernels_ms"], "stats": alone["result"]}
    for limit in LIMITS:
        size = sizes(MAX_ROUNDS, limit)
        nv, nt = size["outVertices"], size["outTriangles"]
        ov, ot = m.DeviceBuffer(ctx, nbytes=12 * nv), m.DeviceBuffer(ctx, nbytes=12 * nt)
        r = best_of(ctx, "kernel.split.", "split.scratch.bytes", split(MAX_ROUNDS, limit, ov, nv, ot, nt))
        r["moved"] = deviation(ov, nv, dv, V, dt, T, limit)         # the output's vertices against the input's surface
        r["lost"] = deviation(dv, V, ov, nv, ot, nt, limit)         # and the other way round
        t = b.Topology()
        b.check(b.lib().mlsgpu_hip_mesh_topology(ctx.h, ot.ptr, nt, nv, C.byref(t)))
        r["manifold_after"] = int(t.manifold)
        if limit == LIMITS[1]:
            r["triangles_behind_round"] = [sizes(k, limit)["outTriangles"] for k in range(1, size["rounds"])]
            target = m.DeviceBuffer(ctx, nbytes=12 * nt)
            then = best_of(ctx, "kernel.flip.", "flip.scratch.bytes", flips(ov, nv, ot, nt, target, MAX_ROUNDS))
            r["then_flips"] = {"kernels_ms": then["kernels_ms"], "stats": then["result"]}
            target.free()
        out["limits"][limit] = r
        ov.free()
        ot.free()
    flipped.free()
    return out


def histogram(f, rows):
    f.write("| | " + " | ".join(str(k) for k in range(16)) + " |\n|" + "---|" * 17 + "\n")
    for name, bins in rows:
        f.write("| %s | " % name + " | ".join(str(x) for x in bins) + " |\n")
    f.write("\n")


def write_notes(f, title, r):
    f.write("### %s: %d vertices, %d triangles\n\n" % (title, r["vertices"], r["triangles"]))
    c = r["classification"]
    f.write("One classification (maxRounds 0), milliseconds, best of five: split %.3f (%s), collapse %.3f (%s).\n\n"
            % (c["split"]["ms"], ", ".join("%s %.3f" % kv for kv in c["split"]["stats"].items()),
               c["collapse"]["ms"], ", ".join("%s %.3f" % kv for kv in c["collapse"]["stats"].items())))
    f.write("To convergence (maxRounds %d), per limit F in grid spacings:\n\n"
            "| F | rounds | splits | boundary | long before | long after | blocked after | vertices after | triangles after | growth | min q before "
            "| min q after | max L before | max L after | moved max | moved rms | lost max | lost rms | manifold after | kernels ms | wall ms "
            "| scratch MB |\n|" % MAX_ROUNDS + "---|" * 22 + "\n")
    for limit, x in r["limits"].items():
        s = x["result"]
        f.write("| %s | %d | %d | %d | %d | %d | %d | %d | %d | %.2f | %.4g | %.4g | %.4g | %.4g | %.3g | %.3g | %.3g | %.3g | %d | %.3f | %.2f | %.1f |\n"
                % (limit, s["rounds"], s["splits"], s["boundarySplits"], s["longBefore"], s["longAfter"], s["blockedAfter"], s["outVertices"],
                   s["outTriangles"], s["outTriangles"] / max(s["numTriangles"], 1), s["minQualityBefore"], s["minQualityAfter"],
                   math.sqrt(s["maxLengthSqBefore"]), math.sqrt(s["maxLengthSqAfter"]), x["moved"]["max"], x["moved"]["rms"], x["lost"]["max"],
                   x["lost"]["rms"], x["manifold_after"], x["kernels_ms"], x["wall_ms"], x["scratch_bytes"] / 1e6))
    f.write("\nMilliseconds per kernel summed over the rounds (launches), best of five:\n\n| F | " + " | ".join(KERNELS) + " |\n|"
            + "---|" * (len(KERNELS) + 1) + "\n")
    for limit, x in r["limits"].items():
        f.write("| %s | " % limit + " | ".join("%.3f (%d)" % (x["stats"].get(k, 0.0), x["launches"].get(k, 0)) for k in KERNELS) + " |\n")
    middle = r["limits"][LIMITS[1]]
    alone, then = r["flips_alone"], middle["then_flips"]
    f.write("\nTriangles behind every round at F = %s: %s.\n" % (LIMITS[1], ", ".join(str(x) for x in middle["triangles_behind_round"])))
    f.write("\nTriangle quality, 16 bins of q from 0 to 1, at F = %s; `flips alone` and `split, flips` are the flips' report after %d "
            "rounds and %d flips (%.3f ms, smallest q %.4g) and after %d rounds and %d flips (%.3f ms, smallest q %.4g):\n\n"
            % (LIMITS[1], alone["stats"]["rounds"], alone["stats"]["flips"], alone["kernels_ms"], alone["stats"]["minQualityAfter"],
               then["stats"]["rounds"], then["stats"]["flips"], then["kernels_ms"], then["stats"]["minQualityAfter"]))
    histogram(f, (("before", middle["result"]["qualityBefore"]), ("split", middle["result"]["qualityAfter"]),
                  ("flips alone", alone["stats"]["qualityAfter"]), ("split, flips", then["stats"]["qualityAfter"])))


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
    fill = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    notes = sys.argv[4] if len(sys.argv) > 4 else None
    import torch

    import mlsgpu_amd as m
    from mlsgpu_amd import binding as b
    from mlsgpu_amd import synth
    device = torch.device("cuda", 0)
    cloud, g = synth.make_cloud_device(cfg, device, scale=1.0, dist=dist)
    sb_t, buckets = synth.bucketize_device(cloud, synth.grid_buckets((g, g, g), 255))
    del cloud
    torch.cuda.synchronize()
    ctx = m.Context(0)
    smax = max(bk.count for bk in buckets)
    scells = max(max(bk.num_vertices) for bk in buckets) - 1
    w = m.Worker(ctx, smax, max_cells=scells, mesh_memory=4096 << 20)
    w.set_keep_splats(True)
    buf = m.DeviceBuffer(ctx, nbytes=sb_t.numel() * 4, borrow=sb_t.data_ptr())
    sink = m.Mesher(ctx, 0.02)
    w.process_batch(buf, buckets, collector=sink.collector(ctx, 0))
    ctx.synchronize()
    chunks = sink.finalize()
    out = {"workload": "%s %s, %d buckets" % (cfg, dist, len(buckets)), "chunks": chunks, "fill_edges": fill}
    out["finalized"] = probe(ctx, m, b, sink.chunk(0, download=False))
    out["fill"] = sink.fill_holes(fill)
    out["filled"] = probe(ctx, m, b, sink.chunk(0, download=False))
    t0 = time.perf_counter()
    out["sink_split_stats"] = sink.split_edges(MAX_ROUNDS, LIMITS[1], 16)
    out["sink_split_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))
    if notes:
        with open(notes, "w") as f:
            f.write("Workload: %s; chunk 0 of %d; fill_holes(%d) filled %d of %d loops; `Mesher.split_edges()` at F = %s on the filled "
                    "sink %.2f ms wall (sized and then written: the rounds run twice).\n\n"
                    % (out["workload"], chunks, fill, out["fill"]["filledLoops"], out["fill"]["loops"], LIMITS[1], out["sink_split_ms"]))
            write_notes(f, "As the weld left it", out["finalized"])
            write_notes(f, "After fill_holes(%d)" % fill, out["filled"])


if __name__ == "__main__":
    main()
