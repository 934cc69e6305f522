#!/usr/bin/env python3
"""The repair of chunk 0 of a finalized, simplified device sink, timed per kernel (HIP events around every launch, the best of
five calls) next to the topology report of the same chunk -- both stages sort 3 T side records, so the report is the
yardstick --, without flags and with MLSGPU_REPAIR_SPLIT_PINCHES; the table goes to the file named last (a Markdown fragment
for profiles/NOTES_repair.md).  repair_probe.py [cfg2|cfg3] [shells|uniform] [cells] [notes.md]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("init", "sides", "sort", "runs", "twins", "marks", "umbrellas", "heads", "vertices", "triangles")
TOPOLOGY = ("init", "classify", "sort", "segments", "twins", "links", "roots")


def best_of(ctx, prefix, scratch, call):
    """The best of five `call`s by the sum of the kernels named prefix*: per-kernel milliseconds, their sum, the wall time of
    the call, and the scratch bytes the stage reported."""
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
        st = {k[len(prefix):]: round(v[0], 4) for k, v in raw.items() if k.startswith(prefix)}
        kernels = sum(st.values())
        if best is None or kernels < best["kernels_ms"]:
            best = {"kernels_ms": round(kernels, 4), "wall_ms": round(wall_ms, 3), "stats": st,
                    "scratch_bytes": raw[scratch][0] / max(raw[scratch][1], 1) if scratch in raw else 0.0}
    best["result"] = result
    return best


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
    cells = float(sys.argv[3]) if len(sys.argv) > 3 else 3.0
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
    finalized = sink.chunk(0, download=False)
    simplified = sink.simplify((-cells, -cells, -cells), cells)
    chunk = sink.chunk(0, download=False)
    V, T = chunk["num_vertices"], chunk["num_triangles"]
    out = {"workload": "%s %s, %d buckets, simplify cell %g" % (cfg, dist, len(buckets), cells), "chunks": chunks,
           "finalized": [finalized["num_vertices"], finalized["num_triangles"]], "simplify": simplified, "vertices": V, "triangles": T,
           "runs": {}}

    def topology():
        t = b.Topology()
        b.check(b.lib().mlsgpu_hip_mesh_topology(ctx.h, chunk["d_triangles"], T, V, C.byref(t)))
        return {"manifold": int(t.manifold), "count": [int(x) for x in t.count], "boundaries": int(t.numBoundaries)}

    out["topology"] = best_of(ctx, "kernel.topology.", "topology.scratch.bytes", topology)
    for name, flags in (("no flags", 0), ("split pinches", b.REPAIR_SPLIT_PINCHES)):
        st = b.RepairStats()
        rc = b.lib().mlsgpu_hip_mesh_repair(ctx.h, chunk["d_vertices"], V, chunk["d_triangles"], T, flags, None, 0, None, 0, None, C.byref(st))
        assert rc in (0, 2), rc
        ov = m.DeviceBuffer(ctx, nbytes=12 * max(st.outVertices, 1))
        ot = m.DeviceBuffer(ctx, nbytes=12 * max(st.outTriangles, 1))

        def repair():
            one = b.RepairStats()
            b.check(b.lib().mlsgpu_hip_mesh_repair(ctx.h, chunk["d_vertices"], V, chunk["d_triangles"], T, flags, ov.ptr, st.outVertices,
                                                   ot.ptr, st.outTriangles, None, C.byref(one)))
            return one.as_dict()

        r = best_of(ctx, "kernel.repair.", "repair.scratch.bytes", repair)
        t = b.Topology()
        b.check(b.lib().mlsgpu_hip_mesh_topology(ctx.h, ot.ptr, st.outTriangles, st.outVertices, C.byref(t)))
        r["manifold_after"] = int(t.manifold)
        out["runs"][name] = r
        ov.free()
        ot.free()
    t0 = time.perf_counter()
    out["sink_repair_stats"] = sink.repair(0)
    out["sink_repair_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    out["sink_manifold_after"] = int(sink.chunk_topology(0).manifold)
    print(json.dumps(out))
    if notes:
        top = out["topology"]
        with open(notes, "w") as f:
            f.write("Workload: %s; chunk 0 of %d: %d vertices, %d triangles finalized, %d and %d simplified; `Mesher.repair()` on the "
                    "sink %.2f ms wall.\n\n" % (out["workload"], chunks, finalized["num_vertices"], finalized["num_triangles"], V, T,
                                                out["sink_repair_ms"]))
            f.write("The topology report of the simplified chunk (manifold %d, counts %s), per-kernel milliseconds, best of five:\n\n"
                    % (top["result"]["manifold"], top["result"]["count"]))
            f.write("| " + " | ".join(TOPOLOGY) + " | kernels | wall | scratch MB |\n|" + "---|" * (len(TOPOLOGY) + 3) + "\n")
            f.write("| " + " | ".join("%.3f" % top["stats"].get(k, 0.0) for k in TOPOLOGY)
                    + " | %.3f | %.2f | %.1f |\n\n" % (top["kernels_ms"], top["wall_ms"], top["scratch_bytes"] / 1e6))
            f.write("One `mlsgpu_hip_mesh_repair` with its outputs in place (the sizes asked for beforehand), per-kernel milliseconds, "
                    "best of five:\n\n")
            f.write("| run | " + " | ".join(KERNELS) + " | kernels | wall | scratch MB | repeated sides | dropped | split | added | "
                    "unused | manifold after |\n")
            f.write("|---|" + "---|" * (len(KERNELS) + 9) + "\n")
            for name, r in out["runs"].items():
                s = r["result"]
                f.write("| %s | " % name + " | ".join("%.3f" % r["stats"].get(k, 0.0) for k in KERNELS)
                        + " | %.3f | %.2f | %.1f | %d | %d | %d | %d | %d | %d |\n"
                        % (r["kernels_ms"], r["wall_ms"], r["scratch_bytes"] / 1e6, s["repeatedSides"], s["droppedTriangles"],
                           s["splitVertices"], s["addedVertices"], s["unusedVertices"], r["manifold_after"]))


if __name__ == "__main__":
    main()
