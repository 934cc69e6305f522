#!/usr/bin/env python3
"""The vertex normals of a finalized device sink, timed per kernel (HIP events around every launch) next to the sink's
finalize, with the plain and the wave-combining accumulate side by side: normals_probe.py [cfg2|cfg3] [shells|uniform]."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
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
    # 12 T of indices read, 36 T of positions gathered, 24 V of sums (the scratch), 12 V of normals written
    algorithmic = 12 * T + 36 * T + 24 * V + 12 * V
    out = {"workload": "%s %s, %d buckets" % (cfg, dist, len(buckets)), "chunks": chunks, "finalize_ms": round(finalize_ms, 2),
           "vertices": V, "triangles": T, "algorithmic_bytes": algorithmic}
    for mode in ("plain", "wave"):
        os.environ["MLSGPU_HIP_NORMALS_ACCUMULATE"] = mode
        m.mesh_normals(ctx, verts, tris)                    # warm-up
        best = None
        for _ in range(5):
            ctx.reset_stats()
            ctx.set_timing(True)
            t0 = time.perf_counter()
            _, stats = m.mesh_normals(ctx, verts, tris)
            wall_ms = (time.perf_counter() - t0) * 1e3      # includes the download of the normals
            ctx.set_timing(False)
            raw = ctx.stats()
            st = {k: round(v[0], 4) for k, v in raw.items() if k.startswith("kernel.normals")}
            kernels = sum(st.values())
            if best is None or kernels < best["kernels_ms"]:
                acc = st.get("kernel.normals.accumulate", 0.0)
                best = {"kernels_ms": round(kernels, 4), "wall_with_download_ms": round(wall_ms, 2), "stats": st,
                        "scratch_bytes": raw["normals.scratch.bytes"][0],
                        "algorithmic_GBps": round(algorithmic / kernels / 1e6, 1) if kernels else None,
                        "accumulate_G_logical_adds_per_s": round(9 * T / acc / 1e6, 2) if acc else None}
        out[mode] = best
    del os.environ["MLSGPU_HIP_NORMALS_ACCUMULATE"]
    out["normals_stats"] = stats
    t0 = time.perf_counter()
    sink.chunk_normals(0, download=False)
    out["sink_chunk_normals_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
