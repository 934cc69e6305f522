#!/usr/bin/env python3
"""The short-edge collapse of chunk 0 of a finalized device sink, as the weld left it and after a simplify, timed per kernel
(HIP events around every launch, the best of five calls) at several edge limits F (in grid spacings): per-kernel totals and
launches of a run to convergence, one classification alone (maxRounds 0) next to the flips' on the same chunk, rounds,
collapses and blocked edges, the two quality histograms, the sizes before and after, how far the result lies from the input
(the deviation report both ways), and the chunk through collapse and then flips against flips alone.
collapse_probe.py [cfg2|cfg3] [shells|uniform] [simplify cells=4] [notes.md]"""
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.flip_probe import best_of  # noqa: E402

KERNELS = ("check", "quality", "records", "sort", "segments", "fixed", "classify", "keys", "apply", "vertices", "triangles")
CLASSIFICATION = {"collapse": ("records", "sort", "segments", "fixed", "classify"), "flip": ("records", "sort", "segments", "classify")}
LIMITS = (0.1, 0.2, 0.3)
MAX_ROUNDS, MIN_COS, MIN_GAIN = 64, 0.5, 1e-6


def probe(ctx, m, b, chunk):
    """Collapse of one chunk where it lies, into buffers of its own, at every limit; flips behind the middle one."""
    V, T = chunk["num_vertices"], chunk["num_triangles"]
    dv = m.DeviceBuffer(ctx, nbytes=12 * V, borrow=chunk["d_vertices"])
    dt = m.DeviceBuffer(ctx, nbytes=12 * T, borrow=chunk["d_triangles"])
    ov, ot, flipped = (m.DeviceBuffer(ctx, nbytes=12 * max(n, 1)) for n in (V, T, T))
    out = {"vertices": V, "triangles": T, "limits": {}}

    def collapse(rounds, limit):
        def call():
            st = b.CollapseStats()
            b.check(b.lib().mlsgpu_hip_mesh_collapse_edges(ctx.h, dv.ptr, V, dt.ptr, T, rounds, limit, MIN_COS, ov.ptr, V, ot.ptr, T, None,
                                                           C.byref(st)))
            return st.as_dict()
        return call

    def flips(vertices, num_vertices, triangles, num_triangles, rounds):
        def call():
            st = b.FlipStats()
            b.check(b.lib().mlsgpu_hip_mesh_flip_edges(ctx.h, vertices.ptr, num_vertices, triangles.ptr, num_triangles, rounds, MIN_GAIN,
                                                       MIN_COS, flipped.ptr, C.byref(st)))
            return st.as_dict()
        return call

    def deviation(points, num_points, vertices, num_vertices, triangles, num_triangles, limit):
        r = b.mesh_deviation(ctx, points, vertices, triangles, limit, want_distances=False, want_nearest=False, num_points=num_points,
                             num_vertices=num_vertices, num_triangles=num_triangles)[2]
        return {"max": math.sqrt(r["maxDistance2"]), "rms": math.sqrt(r["meanSquare"]), "beyond": r["beyond"]}

    once = {"collapse": best_of(ctx, "kernel.collapse.", "collapse.scratch.bytes", collapse(0, LIMITS[1])),
            "flip": best_of(ctx, "kernel.flip.", "flip.scratch.bytes", flips(dv, V, dt, T, 0))}
    out["classification"] = dict((k, {"ms": round(sum(r["stats"].get(n, 0.0) for n in CLASSIFICATION[k]), 4),
                                      "stats": dict((n, r["stats"].get(n, 0.0)) for n in CLASSIFICATION[k])}) for k, r in once.items())
    alone = best_of(ctx, "kernel.flip.", "flip.scratch.bytes", flips(dv, V, dt, T, MAX_ROUNDS))
    out["flips_alone"] = {"kernels_ms": alone["kernels_ms"], "stats": alone["result"]}
    for limit in LIMITS:
        r = best_of(ctx, "kernel.collapse.", "collapse.scratch.bytes", collapse(MAX_ROUNDS, limit))
        s = r["result"]
        r["moved"] = deviation(ov, s["outVertices"], dv, V, dt, T, limit)           # the output's vertices against the input's surface
        r["lost"] = deviation(dv, V, ov, s["outVertices"], ot, s["outTriangles"], limit)   # and the other way round
        t = b.Topology()
        b.check(b.lib().mlsgpu_hip_mesh_topology(ctx.h, ot.ptr, s["outTriangles"], s["outVertices"], C.byref(t)))
        r["manifold_after"] = int(t.manifold)
        if limit == LIMITS[1]:
            then = best_of(ctx, "kernel.flip.", "flip.scratch.bytes", flips(ov, s["outVertices"], ot, s["outTriangles"], MAX_ROUNDS))
            r["then_flips"] = {"kernels_ms": then["kernels_ms"], "stats": then["result"]}
        out["limits"][limit] = r
    for buf in (ov, ot, flipped):
        buf.free()
    return out


def histogram(f, rows):
    f.write("| | " + " | ".join(str(k) for k in range(16)) + " |\n|" + "---|" * 17 + "\n")
    for name, bins in rows:
        f.write("| %s | " % name + " | ".join(str(x) for x in bins) + " |\n")
    f.write("\n")


def write_notes(f, title, r):
    f.write("### %s: %d vertices, %d triangles\n\n" % (title, r["vertices"], r["triangles"]))
    c = r["classification"]
    f.write("One classification (maxRounds 0), milliseconds, best of five: collapse %.3f (%s), flips %.3f (%s).\n\n"
            % (c["collapse"]["ms"], ", ".join("%s %.3f" % kv for kv in c["collapse"]["stats"].items()),
               c["flip"]["ms"], ", ".join("%s %.3f" % kv for kv in c["flip"]["stats"].items())))
    f.write("To convergence (maxRounds %d, minCos %g), per limit F in grid spacings:\n\n"
            "| F | rounds | collapses | short before | blocked after | fixed | vertices after | triangles after | min q before | min q after "
            "| min L2 after | moved max | moved rms | lost max | lost rms | manifold after | kernels ms | wall ms | scratch MB |\n|" % (MAX_ROUNDS, MIN_COS)
            + "---|" * 19 + "\n")
    for limit, x in r["limits"].items():
        s = x["result"]
        f.write("| %s | %d | %d | %d | %d | %d | %d | %d | %.4g | %.4g | %.4g | %.4g | %.4g | %.4g | %.4g | %d | %.3f | %.2f | %.1f |\n"
                % (limit, s["rounds"], s["collapses"], s["shortBefore"], s["blockedAfter"], s["fixedVertices"], s["outVertices"],
                   s["outTriangles"], s["minQualityBefore"], s["minQualityAfter"], s["minLengthSqAfter"], x["moved"]["max"], x["moved"]["rms"],
                   x["lost"]["max"], x["lost"]["rms"], x["manifold_after"], x["kernels_ms"], x["wall_ms"], x["scratch_bytes"] / 1e6))
    f.write("\nMilliseconds per kernel summed over the rounds (launches), best of five:\n\n| F | " + " | ".join(KERNELS) + " |\n|"
            + "---|" * (len(KERNELS) + 1) + "\n")
    for limit, x in r["limits"].items():
        f.write("| %s | " % limit + " | ".join("%.3f (%d)" % (x["stats"].get(k, 0.0), x["launches"].get(k, 0)) for k in KERNELS) + " |\n")
    middle = r["limits"][LIMITS[1]]
    alone, then = r["flips_alone"], middle["then_flips"]
    f.write("\nTriangle quality, 16 bins of q from 0 to 1, at F = %s; `flips alone` and `collapse, flips` are the flips' report after %d "
            "rounds and %d flips (%.3f ms, smallest q %.4g) and after %d rounds and %d flips (%.3f ms, smallest q %.4g):\n\n"
            % (LIMITS[1], alone["stats"]["rounds"], alone["stats"]["flips"], alone["kernels_ms"], alone["stats"]["minQualityAfter"],
               then["stats"]["rounds"], then["stats"]["flips"], then["kernels_ms"], then["stats"]["minQualityAfter"]))
    histogram(f, (("before", middle["result"]["qualityBefore"]), ("collapse", middle["result"]["qualityAfter"]),
                  ("flips alone", alone["stats"]["qualityAfter"]), ("collapse, flips", then["stats"]["qualityAfter"])))


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
    cells = float(sys.argv[3]) if len(sys.argv) > 3 else 4.0
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
    out = {"workload": "%s %s, %d buckets" % (cfg, dist, len(buckets)), "chunks": chunks, "simplify_cell": cells}
    out["finalized"] = probe(ctx, m, b, sink.chunk(0, download=False))
    out["simplify"] = sink.simplify((-cells, -cells, -cells), cells)
    out["simplified"] = probe(ctx, m, b, sink.chunk(0, download=False))
    t0 = time.perf_counter()
    out["sink_collapse_stats"] = sink.collapse_edges(MAX_ROUNDS, LIMITS[1], MIN_COS)
    out["sink_collapse_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))
    if notes:
        with open(notes, "w") as f:
            f.write("Workload: %s; chunk 0 of %d; `Mesher.collapse_edges()` at F = %s on the simplified sink %.2f ms wall.\n\n"
                    % (out["workload"], chunks, LIMITS[1], out["sink_collapse_ms"]))
            write_notes(f, "As the weld left it", out["finalized"])
            write_notes(f, "After a simplify in cells of %g grid spacings" % cells, out["simplified"])


if __name__ == "__main__":
    main()
