#!/usr/bin/env python3
"""The hole filling of chunk 0 of a finalized device sink, timed per kernel (HIP events around every launch, the best of five
calls) next to the sink's finalize, at a small and at the largest maxEdges, and then the same chunk with rectangular blocks of
triangles taken out so that there is something to fill; the table goes to the file named last (a Markdown fragment for
profiles/NOTES_fill.md).  fill_probe.py [cfg2|cfg3] [shells|uniform] [notes.md]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("extent", "init", "classify", "sort", "sides", "loops", "sums", "number", "emit")


def timed(m, ctx, verts, tris, V, T, max_edges):
    """The best of five calls of mesh_fill_holes (each is the size query and the filling call: every kernel before the
    read-back runs twice): per-kernel milliseconds of BOTH calls together, and the statistics."""
    m.mesh_fill_holes(ctx, verts, tris, max_edges, num_vertices=V, num_triangles=T)        # warm-up
    best = None
    for _ in range(5):
        ctx.reset_stats()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        _, _, stats = m.mesh_fill_holes(ctx, verts, tris, max_edges, num_vertices=V, num_triangles=T)
        wall_ms = (time.perf_counter() - t0) * 1e3          # includes the scratch allocations and the download of the result
        ctx.set_timing(False)
        raw = ctx.stats()
        st = {k: round(v[0], 4) for k, v in raw.items() if k.startswith("kernel.fill")}
        kernels = sum(st.values())
        if best is None or kernels < best["kernels_ms"]:
            best = {"kernels_ms": round(kernels, 4), "wall_with_download_ms": round(wall_ms, 2), "stats": st,
                    "scratch_bytes": raw["fill.scratch.bytes"][0] / max(raw["fill.scratch.bytes"][1], 1)}
    best["fill_stats"] = stats
    return best


def punch(tri, every, block):
    """The triangles without `block` consecutive ones out of every `every`: the sink numbers neighbouring triangles close
    together, so a block leaves a few holes of some tens of sides."""
    import numpy as np
    keep = (np.arange(len(tri)) % every) >= block
    return np.ascontiguousarray(tri[keep])


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
    notes = sys.argv[3] if len(sys.argv) > 3 else None
    import numpy as np
    import torch

    import mlsgpu_amd as m
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
    sink.finalize()                                         # warm-up: the slab and the outputs are allocated here
    ctx.synchronize()
    t0 = time.perf_counter()
    chunks = sink.finalize()
    ctx.synchronize()
    finalize_ms = (time.perf_counter() - t0) * 1e3
    chunk = sink.chunk(0, download=False)
    V, T = chunk["num_vertices"], chunk["num_triangles"]
    verts = m.DeviceBuffer(ctx, nbytes=12 * V, borrow=chunk["d_vertices"])
    tris = m.DeviceBuffer(ctx, nbytes=12 * T, borrow=chunk["d_triangles"])
    out = {"workload": "%s %s, %d buckets" % (cfg, dist, len(buckets)), "chunks": chunks, "finalize_ms": round(finalize_ms, 2),
           "vertices": V, "triangles": T, "runs": {}}
    out["runs"]["as finalized, maxEdges 32"] = timed(m, ctx, verts, tris, V, T, 32)
    out["runs"]["as finalized, maxEdges 2^20"] = timed(m, ctx, verts, tris, V, T, 1 << 20)
    punched = m.DeviceBuffer(ctx, array=punch(tris.download(np.uint32, 3 * T).reshape(-1, 3), 4096, 24))
    P = punched.nbytes // 12
    out["runs"]["24 of every 4096 triangles removed (%d left), maxEdges 64" % P] = timed(m, ctx, verts, punched, V, P, 64)
    punched.free()
    t0 = time.perf_counter()
    out["sink_fill_stats"] = sink.fill_holes(32)
    out["sink_fill_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))
    if notes:
        with open(notes, "w") as f:
            f.write("Workload: %s; chunk 0 of %d: %d vertices, %d triangles; finalize %.2f ms; `Mesher.fill_holes(32)` on the sink "
                    "%.2f ms wall.\n\n" % (out["workload"], chunks, V, T, out["finalize_ms"], out["sink_fill_ms"]))
            f.write("Per-kernel milliseconds of one `mesh_fill_holes` of the binding = the size query AND the filling call (the "
                    "kernels up to `sums` run twice), best of five:\n\n")
            f.write("| run | " + " | ".join(KERNELS) + " | kernels | wall with download | scratch MB | boundary sides | loops | "
                    "filled | long | irregular sides |\n")
            f.write("|---|" + "---|" * (len(KERNELS) + 8) + "\n")
            for name, r in out["runs"].items():
                s = r["fill_stats"]
                f.write("| %s | " % name + " | ".join("%.3f" % r["stats"].get("kernel.fill." + k, 0.0) for k in KERNELS)
                        + " | %.3f | %.2f | %.1f | %d | %d | %d | %d | %d |\n"
                        % (r["kernels_ms"], r["wall_with_download_ms"], r["scratch_bytes"] / 1e6, s["boundaryEdges"], s["loops"],
                           s["filledLoops"], s["longLoops"], s["irregularEdges"]))


if __name__ == "__main__":
    main()
