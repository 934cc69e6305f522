#!/usr/bin/env python3
"""The simplifier on the chunk of a finalized device sink, timed per kernel (HIP events around every launch): the mean
placement next to the quadric placement with its wave-combining and its plain accumulate, at cells of 2 and 4 grid spacings:
simplify_probe.py [cfg2|cfg3] [shells|uniform] [cells per cluster side, default 2 4]."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 3


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
    cells = [float(x) for x in sys.argv[3:]] or [2.0, 4.0]
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
           "vertices": V, "triangles": T, "runs": []}
    routes = [("mean", m.mesh_simplify, None), ("quadric wave", m.mesh_simplify_quadric, "wave"),
              ("quadric plain", m.mesh_simplify_quadric, "plain")]
    for cell in cells:
        origin = (-cell, -cell, -cell)                      # vertices are in grid units from the grid's low corner
        for name, call, mode in routes:
            if mode is not None:
                os.environ["MLSGPU_HIP_SIMPLIFY_ACCUMULATE"] = mode
            call(ctx, verts, tris, origin, cell)            # warm-up
            best = None
            for _ in range(REPEATS):
                ctx.reset_stats()
                ctx.set_timing(True)
                t0 = time.perf_counter()
                _, _, stats = call(ctx, verts, tris, origin, cell)
                wall_ms = (time.perf_counter() - t0) * 1e3  # includes the download of the result
                ctx.set_timing(False)
                raw = ctx.stats()
                st = {k: round(v[0], 4) for k, v in raw.items() if k.startswith("kernel.simplify")}
                kernels = sum(st.values())
                if best is None or kernels < best["kernels_ms"]:
                    best = {"cell": cell, "placement": name, "kernels_ms": round(kernels, 4),
                            "wall_with_download_ms": round(wall_ms, 2), "scratch_bytes": raw["simplify.scratch.bytes"][0],
                            "kernels": st, "stats": stats}
            os.environ.pop("MLSGPU_HIP_SIMPLIFY_ACCUMULATE", None)
            out["runs"].append(best)
    print(json.dumps(out))
    names = sorted(set(k for r in out["runs"] for k in r["kernels"]))
    print("%-34s" % "ms" + "".join("%16s" % ("%s @%g" % (r["placement"], r["cell"])) for r in out["runs"]))
    for k in names:
        print("%-34s" % k + "".join("%16.4f" % r["kernels"].get(k, 0.0) for r in out["runs"]))
    print("%-34s" % "all kernels" + "".join("%16.4f" % r["kernels_ms"] for r in out["runs"]))
    print("%-34s" % "simplify.scratch.bytes" + "".join("%16d" % r["scratch_bytes"] for r in out["runs"]))


if __name__ == "__main__":
    main()
