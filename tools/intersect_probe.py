#!/usr/bin/env python3
"""The self-intersection report of chunk 0 of a finalized device sink, timed per kernel (HIP events around every launch, the
best of three calls), plain and after each lossy stage -- a clustering at 4 grid spacings by the mean and by the quadrics, ten
Taubin iterations with a fixed and with a moving boundary, a hole filling -- with the record pairs the pairs kernel looks at per
second and the crossings each mesh has; for scale, the same chunk's topology and deviation reports, timed the same way.  The
table goes to the file named last (a Markdown fragment for profiles/NOTES_intersect.md).
intersect_probe.py [cfg2|cfg3] [shells|uniform] [notes.md]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("extent", "classify", "count", "scan", "emit", "sort", "pairs", "report", "list")
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
    topology = timed(ctx, "kernel.topology", lambda: m.mesh_topology(ctx, tris, V, num_triangles=T))
    sv, st, _ = m.mesh_simplify(ctx, verts, tris, origin, CELL)
    qv, qt, _ = m.mesh_simplify_quadric(ctx, verts, tris, origin, CELL)
    dsv, dst = m.DeviceBuffer(ctx, array=sv), m.DeviceBuffer(ctx, array=st)
    deviation = timed(ctx, "kernel.deviation", lambda: m.mesh_deviation(ctx, dsv, verts, tris, CELL * 3 ** 0.5 / 4, want_distances=False,
                                                                       want_nearest=False, num_points=len(sv), num_vertices=V,
                                                                       num_triangles=T))
    fixed, _ = m.mesh_smooth(ctx, verts, tris, 10, 0.5, -0.53, m.binding.SMOOTH_BOUNDARY_FIXED, num_vertices=V, num_triangles=T)
    curve, _ = m.mesh_smooth(ctx, verts, tris, 10, 0.5, -0.53, m.binding.SMOOTH_BOUNDARY_CURVE, num_vertices=V, num_triangles=T)
    fv, ft, _ = m.mesh_fill_holes(ctx, verts, tris, 64, num_vertices=V, num_triangles=T)
    plain_t = tris.download("uint32", 3 * T).reshape(-1, 3)
    meshes = (("plain", verts, tris, V, T), ("simplify %g" % CELL, dsv, dst, len(sv), len(st)),
              ("simplify-quadric %g" % CELL, qv, qt, len(qv), len(qt)), ("smooth 10 fixed", fixed, plain_t, V, T),
              ("smooth 10 curve", curve, plain_t, V, T), ("fill-holes 64", fv, ft, len(fv), len(ft)))
    out = {"workload": "%s %s, %d buckets" % (cfg, dist, len(buckets)), "chunks": chunks, "vertices": V, "triangles": T,
           "topology_kernels_ms": topology[1], "deviation_kernels_ms": deviation[1], "runs": {}}
    for name, v, t, nv, nt in meshes:
        dv, dt = (a if isinstance(a, m.DeviceBuffer) else m.DeviceBuffer(ctx, array=np.ascontiguousarray(a)) for a in (v, t))
        kernels, total, wall, raw, (_, _, report) = timed(
            ctx, "kernel.intersect", lambda: m.mesh_self_intersections(ctx, dv, dt, want_partners=False, want_pairs=False, num_vertices=nv,
                                                                       num_triangles=nt))
        listed = timed(ctx, "kernel.intersect", lambda: m.mesh_self_intersections(ctx, dv, dt, num_vertices=nv, num_triangles=nt))
        tested, pairs_ms = raw["intersect.pairs.tested"][0], kernels.get("kernel.intersect.pairs", 0.0)
        out["runs"][name] = dict(
            vertices=nv, triangles=nt, kernels=kernels, kernels_ms=total, wall_ms=wall, records=raw["intersect.records"][0],
            cell_size=raw["intersect.cellsize"][0], count_launches=raw["kernel.intersect.count"][1],
            scratch_bytes=raw["intersect.scratch.bytes"][0], tested=tested, tested_per_s=tested / (pairs_ms * 1e-3) if pairs_ms else 0.0,
            candidates_per_s=report["candidatePairs"] / (pairs_ms * 1e-3) if pairs_ms else 0.0, with_list_wall_ms=listed[2],
            list_ms=listed[0].get("kernel.intersect.list", 0.0), report=report)
        for made, given in ((dv, v), (dt, t)):
            if made is not given:
                made.free()
    print(json.dumps(out))
    if notes:
        with open(notes, "w") as f:
            f.write("Workload: %s; chunk 0 of %d: %d vertices, %d triangles.  For scale, on the same chunk in the same session: "
                    "`mesh_topology` %.3f ms and `mesh_deviation` (its clustering's vertices against it, D = a quarter of the cell's "
                    "diagonal) %.3f ms of kernels.\n\n" % (out["workload"], chunks, V, T, topology[1], deviation[1]))
            f.write("Per-kernel milliseconds of one `mesh_self_intersections` without the optional outputs, best of %d (`count` runs "
                    "once per cell size tried); `with list` is the wall time of the binding's two calls that also fetch the partner "
                    "counts and the pair list, `list` their list kernels:\n\n" % REPEATS)
            f.write("| mesh | vertices | triangles | " + " | ".join(KERNELS[:-1]) + " | kernels | wall | with list | list | cell | count launches | "
                    "records | scratch MB | record pairs | candidates | record pairs G/s | candidates G/s | crossing pairs | crossing "
                    "triangles | most partners |\n")
            f.write("|---|" + "---|" * (len(KERNELS) + 16) + "\n")
            for name, r in out["runs"].items():
                s = r["report"]
                f.write("| %s | %d | %d | " % (name, r["vertices"], r["triangles"])
                        + " | ".join("%.3f" % r["kernels"].get("kernel.intersect." + k, 0.0) for k in KERNELS[:-1])
                        + " | %.3f | %.2f | %.2f | %.3f | %.3g | %d | %d | %.1f | %d | %d | %.3f | %.3f | %d | %d | %d |\n"
                        % (r["kernels_ms"], r["wall_ms"], r["with_list_wall_ms"], r["list_ms"], r["cell_size"], r["count_launches"],
                           r["records"], r["scratch_bytes"] / 1e6, r["tested"], s["candidatePairs"], r["tested_per_s"] / 1e9,
                           r["candidates_per_s"] / 1e9, s["crossingPairs"], s["crossingTriangles"], s["maxPartners"]))


if __name__ == "__main__":
    main()
