#!/usr/bin/env python3
"""The deviation report of chunk 0 of a finalized device sink against its own clustering, timed per kernel (HIP events around
every launch, the best of three calls), in both directions and at several search distances, with the pairs the distance kernel
was handed and tested per second; for scale, the same chunk's simplify and topology report, timed the same way.  The table goes
to the file named last (a Markdown fragment for profiles/NOTES_deviation.md).
deviation_probe.py [cfg2|cfg3] [shells|uniform] [notes.md]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("extent", "classify", "count", "scan", "emit", "sort", "pointkeys", "distance", "report")
CELL = 4.0                      # the clustering: 4 grid spacings, as reconstruct --simplify 4
REPEATS = 3


def timed(ctx, prefix, call):
    """The best of REPEATS timed calls: (per-kernel milliseconds under `prefix`, their sum, wall milliseconds, every statistic,
    what the call returned)."""
    call()                                                      # warm-up
    best = None
    for _ in range(REPEATS):
        ctx.reset_stats()
        ctx.set_timing(True)
        t0 = time.perf_counter()
        result = call()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ctx.set_timing(False)
        raw = ctx.stats()
        st = {k: round(v[0], 4) for k, v in raw.items() if k.startswith(prefix)}
        if best is None or sum(st.values()) < best[1]:
            best = (st, round(sum(st.values()), 4), round(wall_ms, 2), raw, result)
    return best


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
    chunks = sink.finalize()
    ctx.synchronize()
    chunk = sink.chunk(0, download=False)
    V, T = chunk["num_vertices"], chunk["num_triangles"]
    verts = m.DeviceBuffer(ctx, nbytes=12 * V, borrow=chunk["d_vertices"])
    tris = m.DeviceBuffer(ctx, nbytes=12 * T, borrow=chunk["d_triangles"])
    origin = (-CELL, -CELL, -CELL)                              # vertices are in grid units from the grid's low corner
    simplify = timed(ctx, "kernel.simplify", lambda: m.mesh_simplify(ctx, verts, tris, origin, CELL))
    topology = timed(ctx, "kernel.topology", lambda: m.mesh_topology(ctx, tris, V, num_triangles=T))
    sv, st, _ = simplify[4]
    dsv, dst = m.DeviceBuffer(ctx, array=sv), m.DeviceBuffer(ctx, array=st)
    out = {"workload": "%s %s, %d buckets" % (cfg, dist, len(buckets)), "chunks": chunks, "vertices": V, "triangles": T,
           "simplified_vertices": len(sv), "simplified_triangles": len(st), "simplify_kernels_ms": simplify[1],
           "topology_kernels_ms": topology[1], "runs": {}}
    diagonal = CELL * 3 ** 0.5
    directions = (("moved", (dsv, verts, tris), dict(num_points=len(sv), num_vertices=V, num_triangles=T)),
                  ("lost", (verts, dsv, dst), dict(num_points=V, num_vertices=len(sv), num_triangles=len(st))))
    for D in (diagonal / 16, diagonal / 4, diagonal):
        for name, arrays, sizes in directions:
            kernels, total, wall, raw, (_, _, report) = timed(
                ctx, "kernel.deviation", lambda: m.mesh_deviation(ctx, *arrays, D, want_distances=False, want_nearest=False, **sizes))
            handed, candidates = raw["deviation.pairs.handed"][0], raw["deviation.pairs.candidates"][0]
            distance_ms = kernels.get("kernel.deviation.distance", 0.0)
            out["runs"]["%s, D = %.3g" % (name, D)] = dict(
                kernels=kernels, kernels_ms=total, wall_ms=wall, grid_pairs=raw["deviation.pairs"][0], cell_size=raw["deviation.cellsize"][0],
                count_launches=raw["kernel.deviation.count"][1], lanes=raw["deviation.lanes"][0], scratch_bytes=raw["deviation.scratch.bytes"][0], handed=handed,
                candidates=candidates, handed_per_s=handed / (distance_ms * 1e-3) if distance_ms else 0.0,
                candidates_per_s=candidates / (distance_ms * 1e-3) if distance_ms else 0.0, report=report)
    print(json.dumps(out))
    if notes:
        with open(notes, "w") as f:
            f.write("Workload: %s; chunk 0 of %d: %d vertices, %d triangles; its `mesh_simplify` at cell %g: %d vertices, %d triangles.  "
                    "For scale, on the same chunk in the same session: `mesh_simplify` %.3f ms and `mesh_topology` %.3f ms of kernels.\n\n"
                    % (out["workload"], chunks, V, T, CELL, len(sv), len(st), simplify[1], topology[1]))
            f.write("Per-kernel milliseconds of one `mesh_deviation` without the optional outputs, best of %d (`count` runs once per "
                    "cell size tried; `sort` is both sorts):\n\n" % REPEATS)
            f.write("| run | " + " | ".join(KERNELS) + " | kernels | wall | lanes per point | cell | count launches | grid pairs | scratch MB | pairs handed | "
                    "candidates | handed G/s | candidates G/s | within | beyond | max distance |\n")
            f.write("|---|" + "---|" * (len(KERNELS) + 14) + "\n")
            for name, r in out["runs"].items():
                s = r["report"]
                f.write("| %s | " % name + " | ".join("%.3f" % r["kernels"].get("kernel.deviation." + k, 0.0) for k in KERNELS)
                        + " | %.3f | %.2f | %d | %.3g | %d | %d | %.1f | %d | %d | %.2f | %.2f | %d | %d | %.4g |\n"
                        % (r["kernels_ms"], r["wall_ms"], r["lanes"], r["cell_size"], r["count_launches"], r["grid_pairs"], r["scratch_bytes"] / 1e6,
                           r["handed"], r["candidates"], r["handed_per_s"] / 1e9, r["candidates_per_s"] / 1e9, s["within"], s["beyond"],
                           s["maxDistance2"] ** 0.5))


if __name__ == "__main__":
    main()
