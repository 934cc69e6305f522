#!/usr/bin/env python3
"""The simplifier on a finalized device sink, timed per kernel (HIP events around every launch) next to the sink's finalize:
simplify_probe.py [cfg2|cfg3] [shells|uniform] [cells per cluster side = 4]."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
    cell = float(sys.argv[3]) if len(sys.argv) > 3 else 4.0
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
    origin = (-cell, -cell, -cell)                          # vertices are in grid units from the grid's low corner
    sink.finalize()
    sink.simplify(origin, cell)                             # warm-up; a finalize brings the whole chunk back
    ctx.synchronize()
    t0 = time.perf_counter()
    chunks = sink.finalize()
    ctx.synchronize()
    finalize_ms = (time.perf_counter() - t0) * 1e3
    ctx.reset_stats()
    ctx.set_timing(True)
    t0 = time.perf_counter()
    stats = sink.simplify(origin, cell)
    wall_ms = (time.perf_counter() - t0) * 1e3
    ctx.set_timing(False)
    st = {k: round(v[0], 3) for k, v in ctx.stats().items() if k.startswith(("kernel.simplify", "simplify."))}
    kernels = sum(v for k, v in st.items() if k.startswith("kernel."))
    topo = sink.chunk_topology(0)
    print(json.dumps({"workload": "%s %s, %d buckets" % (cfg, dist, len(buckets)), "chunks": chunks, "cell": cell,
                      "finalize_ms": round(finalize_ms, 2), "simplify_wall_ms": round(wall_ms, 2),
                      "simplify_kernels_ms": round(kernels, 3), "stats": st, "simplify": stats,
                      "manifold_after": int(topo.manifold), "counts_after": [int(x) for x in topo.count]}))


if __name__ == "__main__":
    main()
