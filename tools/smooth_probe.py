#!/usr/bin/env python3
"""The Taubin smoothing of chunk 0 of a finalized device sink, timed per kernel (HIP events around every launch, the best of
five calls) next to the sink's finalize: the adjacency build kernel by kernel, one pass, the pass's algorithmic bytes and the
rate against them, with the serial and the batched pass kernel side by side.  smooth_probe.py [cfg2|cfg3] [shells|uniform] [iterations=10]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BUILD = ("load", "records", "sort", "mark", "adjacency")


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
    iterations = int(sys.argv[3]) if len(sys.argv) > 3 else 10
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
           "vertices": V, "triangles": T, "iterations": iterations}
    for kernel in ("serial", "batched"):
        os.environ["MLSGPU_HIP_SMOOTH_PASS"] = kernel
        m.mesh_smooth(ctx, verts, tris, iterations, 0.5, -0.53)     # warm-up
        best = None
        for _ in range(5):
            ctx.reset_stats()
            ctx.set_timing(True)
            t0 = time.perf_counter()
            _, stats = m.mesh_smooth(ctx, verts, tris, iterations, 0.5, -0.53)
            wall_ms = (time.perf_counter() - t0) * 1e3      # includes the scratch allocation and the download of the result
            ctx.set_timing(False)
            raw = ctx.stats()
            st = {k: round(v[0], 4) for k, v in raw.items() if k.startswith("kernel.smooth")}
            kernels = sum(st.values())
            if best is None or kernels < best["kernels_ms"]:
                passes = raw["kernel.smooth.pass"][1]
                best = {"kernels_ms": round(kernels, 4), "wall_with_download_ms": round(wall_ms, 2), "stats": st,
                        "build_ms": round(sum(st.get("kernel.smooth." + k, 0.0) for k in BUILD), 4),
                        "pass_ms": round(st["kernel.smooth.pass"] / passes, 4), "passes": passes,
                        "scratch_bytes": raw["smooth.scratch.bytes"][0]}
        # a pass: per vertex its own 16-byte row and its 8-byte run read and a 16-byte row written; per neighbour a 4-byte
        # index and a gathered 16-byte row.  Neighbours: both ends of every edge, less the boundary vertices' under FIXED (2 E
        # bounds it)
        neighbours = 2 * stats["numEdges"]
        algorithmic = 40 * V + 20 * neighbours
        best["pass_algorithmic_bytes"] = algorithmic
        best["pass_algorithmic_GBps"] = round(algorithmic / best["pass_ms"] / 1e6, 1)
        best["pass_G_neighbours_per_s"] = round(neighbours / best["pass_ms"] / 1e6, 2)
        out[kernel] = best
    del os.environ["MLSGPU_HIP_SMOOTH_PASS"]
    out["smooth_stats"] = stats
    t0 = time.perf_counter()
    sink.smooth(iterations)
    out["sink_smooth_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
