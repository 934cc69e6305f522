#!/usr/bin/env python3
"""The compact read-back of every chunk of a finalized device sink at 16 and at 32 vertex bits: the encoder timed per kernel
(HIP events around every launch), the blob's bytes against the raw arrays', the width histogram, the copy of the raw arrays
against the copy of the blob (both into pinned memory), the host decoder on 1, 8 and 16 threads, and the whole route -- encode,
copy, decode -- against the raw copy alone.  Every time is the best of REPEATS after a warm-up, host clock around work that
ends in a synchronise.  The tables go to the file named last (a Markdown fragment for profiles/NOTES_compact.md).
compact_probe.py [cfg2|cfg3] [shells|uniform] [notes.md]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("extent", "plan", "scan", "header", "vertices", "triangles")
REPEATS = 5
THREADS = (1, 8, 16)


def best_ms(call, repeats=REPEATS):
    call()                                                      # warm-up
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None or ms < best else best
    return best


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    dist = sys.argv[2] if len(sys.argv) > 2 else "shells"
    notes = sys.argv[3] if len(sys.argv) > 3 else None
    import numpy as np
    import torch

    import mlsgpu_amd as m
    from mlsgpu_amd import binding as b, synth
    L = b.lib()
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
    out = {"workload": "%s %s, %d buckets" % (cfg, dist, len(buckets)), "chunks": chunks, "runs": []}
    for i in range(chunks):
        chunk = sink.chunk(i, download=False)
        V, T = chunk["num_vertices"], chunk["num_triangles"]
        raw_bytes = 12 * (V + T)
        pinned_raw, pinned_blob = b.PinnedBuffer(raw_bytes + 64), b.PinnedBuffer(raw_bytes + 4096)
        verts = np.empty((V, 3), np.float32)
        tris = np.empty((T, 3), np.uint32)

        def copy_raw():
            b.check(L.mlsgpu_hip_memcpy_d2h(ctx.h, pinned_raw.ptr, chunk["d_vertices"], 12 * V, 1))
            b.check(L.mlsgpu_hip_memcpy_d2h(ctx.h, pinned_raw.ptr + 12 * V, chunk["d_triangles"], 12 * T, 1))
            ctx.synchronize()

        raw_ms = best_ms(copy_raw)
        reference = np.ctypeslib.as_array(C.cast(pinned_raw.ptr, C.POINTER(C.c_uint32)), (3 * (V + T),)).copy()
        for bits in (16, 32):
            st = b.CompactStats()
            args = (ctx.h, chunk["d_vertices"], V, chunk["d_triangles"], T, bits)
            rc = L.mlsgpu_hip_mesh_compact(*args, None, 0, C.byref(st))
            assert rc == 2, rc
            blob_bytes = int(st.blobBytes)
            dblob = b.DeviceBuffer(ctx, nbytes=blob_bytes)

            def encode():
                b.check(L.mlsgpu_hip_mesh_compact(*args, dblob.ptr, blob_bytes, C.byref(st)))

            encode_ms = best_ms(encode)
            kernels = None
            for _ in range(REPEATS):
                ctx.reset_stats()
                ctx.set_timing(True)
                encode()
                ctx.set_timing(False)
                rawstats = ctx.stats()
                k = {name: round(rawstats.get("kernel.compact." + name, (0.0, 0))[0], 4) for name in KERNELS}
                if kernels is None or sum(k.values()) < sum(kernels.values()):
                    kernels, scratch = k, rawstats.get("compact.scratch.bytes", (0.0, 0))[0]

            def copy_blob():
                b.check(L.mlsgpu_hip_memcpy_d2h(ctx.h, pinned_blob.ptr, dblob.ptr, blob_bytes, 1))
                ctx.synchronize()

            blob_ms = best_ms(copy_blob)
            decode_ms = {}
            for threads in THREADS:
                decode_ms[threads] = best_ms(lambda: b.check(L.mlsgpu_hip_compact_decode(pinned_blob.ptr, blob_bytes, b._p(verts), b._p(tris),
                                                                                        threads)))
            assert tris.reshape(-1).tobytes() == reference[3 * V:].tobytes()
            if bits == 32:
                assert verts.view(np.uint32).reshape(-1).tobytes() == reference[:3 * V].tobytes()

            def route():
                b.check(L.mlsgpu_hip_mesher_chunk_compact(sink.h, i, bits, pinned_blob.ptr, pinned_blob.nbytes, C.byref(st)))
                b.check(L.mlsgpu_hip_compact_decode(pinned_blob.ptr, blob_bytes, b._p(verts), b._p(tris), THREADS[-1]))

            route_ms = best_ms(route)
            d = st.as_dict()
            out["runs"].append(dict(chunk=i, bits=bits, vertices=V, triangles=T, raw_bytes=raw_bytes, blob_bytes=blob_bytes,
                                    vertex_bytes=d["vertexBytes"], triangle_bytes=d["triangleBytes"], exceptions=d["exceptions"],
                                    groups=d["groups"], histogram={str(k): n for k, n in enumerate(d["widthHistogram"]) if n},
                                    step=d["step"], kernels=kernels, kernels_ms=round(sum(kernels.values()), 4), scratch_bytes=scratch,
                                    encode_ms=round(encode_ms, 3), raw_copy_ms=round(raw_ms, 3), blob_copy_ms=round(blob_ms, 3),
                                    decode_ms={str(k): round(v, 3) for k, v in decode_ms.items()}, route_ms=round(route_ms, 3)))
            dblob.free()
        pinned_raw.free()
        pinned_blob.free()
    print(json.dumps(out))
    if notes:
        with open(notes, "w") as f:
            f.write("Workload: %s; %d chunk(s).  Milliseconds, best of %d after a warm-up.\n\n" % (out["workload"], chunks, REPEATS))
            f.write("| chunk | bits | vertices | triangles | raw MB | blob MB | ratio | vertex ratio | triangle ratio | exceptions / triangle | "
                    + " | ".join(KERNELS) + " | kernels | encode call | scratch KB |\n")
            f.write("|---|" + "---|" * (len(KERNELS) + 12) + "\n")
            for r in out["runs"]:
                f.write("| %d | %d | %d | %d | %.2f | %.2f | %.3f | %.3f | %.3f | %.4f | " % (
                    r["chunk"], r["bits"], r["vertices"], r["triangles"], r["raw_bytes"] / 1e6, r["blob_bytes"] / 1e6,
                    r["blob_bytes"] / max(r["raw_bytes"], 1), r["vertex_bytes"] / max(12 * r["vertices"], 1),
                    r["triangle_bytes"] / max(12 * r["triangles"], 1), r["exceptions"] / max(r["triangles"], 1))
                    + " | ".join("%.3f" % r["kernels"][k] for k in KERNELS)
                    + " | %.3f | %.3f | %.1f |\n" % (r["kernels_ms"], r["encode_ms"], r["scratch_bytes"] / 1e3))
            f.write("\n| chunk | bits | raw copy | raw GB/s | blob copy | blob GB/s | "
                    + " | ".join("decode %d" % t for t in THREADS) + " | decode GB/s of raw (%d threads) | route (encode + copy + decode %d) | "
                    "route / raw copy |\n" % (THREADS[-1], THREADS[-1]))
            f.write("|---|" + "---|" * (len(THREADS) + 8) + "\n")
            for r in out["runs"]:
                f.write("| %d | %d | %.3f | %.1f | %.3f | %.1f | " % (r["chunk"], r["bits"], r["raw_copy_ms"],
                                                                      r["raw_bytes"] / r["raw_copy_ms"] / 1e6, r["blob_copy_ms"],
                                                                      r["blob_bytes"] / r["blob_copy_ms"] / 1e6)
                        + " | ".join("%.3f" % r["decode_ms"][str(t)] for t in THREADS)
                        + " | %.2f | %.3f | %.2f |\n" % (r["raw_bytes"] / r["decode_ms"][str(THREADS[-1])] / 1e6, r["route_ms"],
                                                         r["route_ms"] / r["raw_copy_ms"]))
            f.write("\nWidth histograms (groups per width):\n\n")
            for r in out["runs"]:
                if r["bits"] == 32:
                    f.write("- chunk %d, %d groups: %s\n" % (r["chunk"], r["groups"],
                                                             ", ".join("w=%s: %d" % kv for kv in r["histogram"].items())))


if __name__ == "__main__":
    main()
