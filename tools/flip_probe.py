#!/usr/bin/env python3
"""The Delaunay edge flips of chunk 0 of a finalized device sink, as the weld left it and after a simplify, timed per kernel
(HIP events around every launch, the best of five calls) next to the topology report of the same chunk -- both stages sort
3 T side records, the flips once per round: per-kernel totals and launches of a run to convergence, the run cut off after
0, 1, 2, 4, 8 and 16 rounds (what a round costs as the candidates thin out), rounds, flips and the two quality histograms.
flip_probe.py [cfg2|cfg3] [shells|uniform] [simplify cells=4] [notes.md]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("check", "quality", "records", "sort", "segments", "classify", "keys", "apply")
TOPOLOGY = ("init", "classify", "sort", "segments", "twins", "links", "roots")
MAX_ROUNDS, MIN_GAIN, MIN_COS = 64, 1e-6, 0.5


def best_of(ctx, prefix, scratch, call):
    """The best of five `call`s by the sum of the kernels named prefix*: per-kernel milliseconds (the sort's launches under
    one name) and launches, their sum, the wall time of the call, and the scratch bytes the stage reported."""
    call()                                                  # warm-up
    best = None
    for _ in range(5):
        ctx.reset_stats()
        ctx.set_timing(True)
        ctx.synchronize()
        t0 = time.perf_counter()
        result = call()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ctx.set_timing(False)
        raw = ctx.stats()
        st, launches = {}, {}
        for k, v in raw.items():
            if k.startswith(prefix):
                name = k[len(prefix):].split(".")[0]
                st[name] = round(st.get(name, 0.0) + v[0], 4)
                launches[name] = launches.get(name, 0) + int(v[1])
        kernels = sum(st.values())
        if best is None or kernels < best["kernels_ms"]:
            best = {"kernels_ms": round(kernels, 4), "wall_ms": round(wall_ms, 3), "stats": st, "launches": launches,
                    "scratch_bytes": raw[scratch][0] / max(raw[scratch][1], 1) if scratch in raw else 0.0}
    best["result"] = result
    return best


def probe(ctx, m, b, chunk):
    """Topology report and flips of one chunk where it lies; the flips write to a buffer of their own."""
    V, T = chunk["num_vertices"], chunk["num_triangles"]
    out = {"vertices": V, "triangles": T}

    def topology():
        t = b.Topology()
        b.check(b.lib().mlsgpu_hip_mesh_topology(ctx.h, chunk["d_triangles"], T, V, C.byref(t)))
        return {"manifold": int(t.manifold), "boundaries": int(t.numBoundaries), "edges": int(t.edges)}

    out["topology"] = best_of(ctx, "kernel.topology.", "topology.scratch.bytes", topology)
    ot = m.DeviceBuffer(ctx, nbytes=12 * max(T, 1))

    def flips(rounds):
        def call():
            st = b.FlipStats()
            b.check(b.lib().mlsgpu_hip_mesh_flip_edges(ctx.h, chunk["d_vertices"], V, chunk["d_triangles"], T, rounds, MIN_GAIN, MIN_COS,
                                                       ot.ptr, C.byref(st)))
            return st.as_dict()
        return call

    out["flip"] = best_of(ctx, "kernel.flip.", "flip.scratch.bytes", flips(MAX_ROUNDS))
    out["cut_off"] = {}
    for rounds in (0, 1, 2, 4, 8, 16):
        r = best_of(ctx, "kernel.flip.", "flip.scratch.bytes", flips(rounds))
        out["cut_off"][rounds] = {"kernels_ms": r["kernels_ms"], "wall_ms": r["wall_ms"], "flips": r["result"]["flips"],
                                  "nonDelaunayAfter": r["result"]["nonDelaunayAfter"], "classify_ms": r["stats"].get("classify", 0.0),
                                  "sort_ms": r["stats"].get("sort", 0.0)}
    t = b.Topology()
    b.check(b.lib().mlsgpu_hip_mesh_topology(ctx.h, ot.ptr, T, V, C.byref(t)))
    out["manifold_after"] = int(t.manifold)
    ot.free()
    return out


def write_notes(f, title, r):
    top, flip, s = r["topology"], r["flip"], r["flip"]["result"]
    f.write("### %s: %d vertices, %d triangles\n\n" % (title, r["vertices"], r["triangles"]))
    f.write("Topology report (manifold %d, %d boundaries), per-kernel milliseconds, best of five:\n\n"
            % (top["result"]["manifold"], top["result"]["boundaries"]))
    f.write("| " + " | ".join(TOPOLOGY) + " | kernels | wall | scratch MB |\n|" + "---|" * (len(TOPOLOGY) + 3) + "\n")
    f.write("| " + " | ".join("%.3f" % top["stats"].get(k, 0.0) for k in TOPOLOGY)
            + " | %.3f | %.2f | %.1f |\n\n" % (top["kernels_ms"], top["wall_ms"], top["scratch_bytes"] / 1e6))
    f.write("Edge flips to convergence (maxRounds %d, minGain %g, minCos %g): %d rounds, %d flips, converged %d, non-Delaunay %d -> %d, "
            "blocked %d, interior edges %d of %d, manifold after %d.  Milliseconds summed over the rounds (launches), best of five:\n\n"
            % (MAX_ROUNDS, MIN_GAIN, MIN_COS, s["rounds"], s["flips"], s["converged"], s["nonDelaunayBefore"], s["nonDelaunayAfter"],
               s["blockedAfter"], s["interiorEdges"], s["numEdges"], r["manifold_after"]))
    f.write("| " + " | ".join(KERNELS) + " | kernels | wall | scratch MB |\n|" + "---|" * (len(KERNELS) + 3) + "\n")
    f.write("| " + " | ".join("%.3f (%d)" % (flip["stats"].get(k, 0.0), flip["launches"].get(k, 0)) for k in KERNELS)
            + " | %.3f | %.2f | %.1f |\n\n" % (flip["kernels_ms"], flip["wall_ms"], flip["scratch_bytes"] / 1e6))
    f.write("Cut off after R rounds (R + 1 classifications):\n\n| R | kernels ms | wall ms | sort ms | classify ms | flips | non-Delaunay left |\n"
            "|---|---|---|---|---|---|---|\n")
    for rounds, c in r["cut_off"].items():
        f.write("| %s | %.3f | %.2f | %.3f | %.3f | %d | %d |\n" % (rounds, c["kernels_ms"], c["wall_ms"], c["sort_ms"], c["classify_ms"],
                                                                  c["flips"], c["nonDelaunayAfter"]))
    f.write("\nTriangle quality, 16 bins of q from 0 to 1; the smallest q %.6g -> %.6g:\n\n| | " % (s["minQualityBefore"], s["minQualityAfter"])
            + " | ".join(str(k) for k in range(16)) + " |\n|" + "---|" * 17 + "\n")
    for name in ("qualityBefore", "qualityAfter"):
        f.write("| %s | " % name[7:].lower() + " | ".join(str(x) for x in s[name]) + " |\n")
    f.write("\n")


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
    out["sink_flip_stats"] = sink.flip_edges(MAX_ROUNDS, MIN_GAIN, MIN_COS)
    out["sink_flip_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))
    if notes:
        with open(notes, "w") as f:
            f.write("Workload: %s; chunk 0 of %d; `Mesher.flip_edges()` on the simplified sink %.2f ms wall.\n\n"
                    % (out["workload"], chunks, out["sink_flip_ms"]))
            write_notes(f, "As the weld left it", out["finalized"])
            write_notes(f, "After a simplify in cells of %g grid spacings" % cells, out["simplified"])


if __name__ == "__main__":
    main()
