"""The device edge flips (mlsgpu_hip_mesh_flip_edges, mlsgpu_hip_mesher_flip_edges, reconstruct --flip-edges) against the CPU
oracle of flip_cases.py: every triangle row and every statistic, bit for bit.  test_flip_oracle.py checks on the CPU that the
inputs used here converge within MAX_ROUNDS and that the ones called free of ties are."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import flip_cases as fc
import normals_cases as nc
import smooth_cases as sc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_ROUNDS = 64


def run(ctx, vertices, triangles, max_rounds=MAX_ROUNDS, min_gain=fc.MIN_GAIN, min_cos=fc.MIN_COS, **kw):
    from mlsgpu_amd import binding as b
    return b.mesh_flip_edges(ctx, vertices, (np.asarray(triangles, np.int64) & 0xFFFFFFFF).astype(np.uint32), max_rounds, min_gain,
                             min_cos, **kw)


def check(ctx, vertices, triangles, max_rounds=MAX_ROUNDS, min_gain=fc.MIN_GAIN, min_cos=fc.MIN_COS):
    want = fc.flip(vertices, triangles, max_rounds, min_gain, min_cos)
    fc.assert_same(run(ctx, vertices, triangles, max_rounds, min_gain, min_cos), want)
    return want


# ---------------------------------------------------------------- hand cases and empty meshes

def test_hand_cases_and_empty_meshes(ctx):
    p, tri = fc.kite()
    out, st = run(ctx, p, tri)
    assert out.tolist() == [[0, 3, 2], [1, 2, 3]]
    assert (st["numEdges"], st["interiorEdges"], st["rounds"], st["flips"], st["converged"]) == (5, 1, 2, 1, 1)
    assert (st["nonDelaunayBefore"], st["nonDelaunayAfter"], st["blockedAfter"]) == (1, 0, 0)
    for build in (fc.kite, fc.square, fc.tetrahedron, fc.pillow, fc.folded, fc.concave, fc.cap):
        p, tri = build()
        for min_gain, min_cos in ((fc.MIN_GAIN, 0.5), (0.0, -1.0)):
            for rounds in (0, 1, MAX_ROUNDS):
                check(ctx, p, tri, rounds, min_gain, min_cos)
    assert check(ctx, *fc.cap())[0].tolist() == [[0, 3, 2], [1, 2, 3]]
    assert check(ctx, *fc.folded(), min_cos=-1.0)[1]["flips"] == 1 and check(ctx, *fc.concave(), min_cos=-1.0)[1]["blockedAfter"] == 1
    p, tri = fc.flat_grid(4, 4, 0.3, 1)
    out, st = check(ctx, p, tri, 0)                                 # maxRounds = 0: a pure report, the output a copy
    assert out.tolist() == tri.tolist() and st["numEdges"] == 33 and st["qualityBefore"] == st["qualityAfter"]
    none = dict(fc.empty_stats(), rounds=1, converged=1)            # no triangle takes part: the first round finds no winner
    assert check(ctx, p[:0], tri[:0])[1] == none and check(ctx, p[:0], tri[:0], 0)[1] == fc.empty_stats()
    out, st = check(ctx, p, tri[:0])                                # T = 0
    assert len(out) == 0 and st == dict(none, numVertices=16) and check(ctx, p, tri[:0], 0)[1]["rounds"] == 0
    out, st = check(ctx, p[:0], tri)                                # V = 0: every index is out of range, the rows stay
    assert out.tolist() == tri.tolist() and st == dict(none, numTriangles=18, outOfRangeTriangles=18)
    assert check(ctx, p[:0], tri, 0)[0].tolist() == tri.tolist()


def test_classification_order(ctx):
    """An index >= V wins over a vertex twice, as for the smoothing."""
    import topology_cases as tc
    p, tri = tc.classification_trap()
    out, st = check(ctx, p, tri)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["numEdges"], st["interiorEdges"]) == (2, 1, 5, 1)
    assert out[2:].tolist() == tri[2:].tolist()


# ---------------------------------------------------------------- grids

def test_flat_and_bumpy_grids(ctx):
    _, st = check(ctx, *fc.flat_grid(40, 40, 0.3, 1))
    assert st["converged"] == 1 and st["nonDelaunayAfter"] == 0 and st["minQualityAfter"] > st["minQualityBefore"] and st["flips"] > 300
    _, st = check(ctx, *fc.grid_mesh(40, 40, jitter=0.45, seed=2))
    assert st["converged"] == 1 and st["nonDelaunayAfter"] == st["blockedAfter"] > 0
    for rounds in (0, 1, 3):                                        # the cap on the rounds
        assert check(ctx, *fc.flat_grid(40, 40, 0.3, 1), rounds)[1]["converged"] == 0
    check(ctx, *fc.flat_grid(40, 40, 0.3, 1), MAX_ROUNDS, 0.25, 1.0)      # another gain; minCos 1 blocks what is not flat to the bit


@pytest.fixture(scope="module")
def big_grid():
    p, tri = fc.grid_mesh(300, 300, jitter=0.3, seed=11)
    assert p.shape == (90_000, 3) and tri.shape == (178_802, 3)
    return p, tri, fc.flip(p, tri, MAX_ROUNDS)


def test_several_sort_tiles(ctx, big_grid):
    p, tri, want = big_grid
    fc.assert_same(run(ctx, p, tri), want)
    assert want[1]["converged"] == 1 and want[1]["flips"] > 10_000 and want[1]["blockedAfter"] > 0
    assert 3 * len(tri[:-1]) % 64 != 0 and len(tri[:-1]) % 64 != 0 and len(p) % 64 != 0       # a partial last wave
    check(ctx, p, tri[:-1])


# ---------------------------------------------------------------- one hub

def test_fan_around_one_hub(ctx):
    """One hub of valence 20 000: every spoke is an interior edge with the hub among its four vertices, so thousands of
    candidates send to one address and exactly one wins a round."""
    p, tri = nc.fan_mesh(20_000, seed=1)
    _, st = check(ctx, p, tri, 3)
    assert (st["interiorEdges"], st["rounds"], st["flips"], st["converged"]) == (20_000, 3, 3, 0) and st["nonDelaunayBefore"] > 2000


# ---------------------------------------------------------------- closed surface, scaling

def test_closed_torus_and_scaling(ctx):
    from mlsgpu_amd import binding as b
    import topology_cases as tc
    p, tri = sc.noisy_torus(200, 40, 0.004, 7)
    out, st = check(ctx, p, tri)
    assert st["converged"] == 1 and st["flips"] > 100 and st["numEdges"] == st["interiorEdges"] == 24_000
    before = tc.report_fields(b.mesh_topology(ctx, tri.astype(np.uint32), len(p)))
    assert before["manifold"] == 1 and tc.report_fields(b.mesh_topology(ctx, out, len(p))) == before
    for shift in (-7, 40, -60):
        s = np.float32(2.0) ** np.float32(shift)
        fc.assert_same(run(ctx, p * s, tri), (out, st))


# ---------------------------------------------------------------- counters, guard bands, aliasing

def test_counters_guard_bands_and_in_place(ctx):
    from mlsgpu_amd import binding as b
    p, tri = fc.defect_mesh()
    assert (tri == 0xFFFFFFFF).sum() == 1
    want = check(ctx, p, tri)
    assert (want[1]["outOfRangeTriangles"], want[1]["degenerateTriangles"]) == (2, 2) and want[1]["flips"] > 3
    dead = [5, 77, 20, 121]
    assert want[0][dead].tolist() == (tri[dead] & 0xFFFFFFFF).tolist()      # dead rows keep their bits
    T, G = len(tri), 1024
    rows = (tri & 0xFFFFFFFF).astype(np.uint32)
    band = np.full(2 * G + 3 * T, 0xABCD1234, np.uint32)
    dv, dt = b.DeviceBuffer(ctx, array=p), b.DeviceBuffer(ctx, array=rows)
    out = b.DeviceBuffer(ctx, array=band)
    st = b.FlipStats()
    b.check(b.lib().mlsgpu_hip_mesh_flip_edges(ctx.h, dv.ptr, len(p), dt.ptr, T, MAX_ROUNDS, fc.MIN_GAIN, fc.MIN_COS, out.ptr + 4 * G, C.byref(st)))
    got = out.download(np.uint32)
    assert (got[:G] == 0xABCD1234).all() and (got[G + 3 * T:] == 0xABCD1234).all()
    fc.assert_same((got[G:G + 3 * T], st.as_dict()), want)
    assert dt.download(np.uint32).tobytes() == rows.tobytes()       # the input is left alone ...
    assert dv.download(np.float32).tobytes() == p.tobytes()
    b.check(b.lib().mlsgpu_hip_mesh_flip_edges(ctx.h, dv.ptr, len(p), dt.ptr, T, MAX_ROUNDS, fc.MIN_GAIN, fc.MIN_COS, dt.ptr, C.byref(st)))
    fc.assert_same((dt.download(np.uint32), st.as_dict()), want)    # ... unless it is the output
    for buf in (dv, dt, out):
        buf.free()
    fc.assert_same(run(ctx, p, tri, in_place=True), want)


# ---------------------------------------------------------------- determinism

def test_determinism(ctx, big_grid):
    p, tri, want = big_grid
    a, b = run(ctx, p, tri), run(ctx, p, tri)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    order = np.random.default_rng(3).permutation(len(tri))          # a permutation of the triangles permutes the output
    fc.assert_same(run(ctx, p, tri[order]), (want[0][order], want[1]))
    turns = np.random.default_rng(4).integers(0, 3, len(tri))       # rotated corners: the same set of triangles
    turned = np.stack([tri[np.arange(len(tri)), (turns + k) % 3] for k in range(3)], axis=1)
    out, st = run(ctx, p, turned)
    assert st == want[1] and fc.triangle_set(out).tolist() == fc.triangle_set(want[0]).tolist()
    p, tri = fc.flat_grid(40, 40, 0.3, 1)                           # free of ties: renumbering the vertices renumbers the result
    want = fc.flip(p, tri, MAX_ROUNDS)
    q, qtri, perm = fc.renumbered(p, tri, 5)
    out, st = run(ctx, q, qtri)
    assert st == want[1] and fc.triangle_set(out).tolist() == fc.triangle_set(perm[want[0].astype(np.int64)]).tolist()


# ---------------------------------------------------------------- errors

def small_correct_call(ctx):
    check(ctx, *fc.flat_grid(9, 11, 0.3, 3))


def test_errors_leave_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    p, tri = fc.flat_grid(9, 11, 0.3, 3)
    p[40, 1] = np.nan
    p[60, 0] = np.inf
    with pytest.raises(fc.Invalid, match="vertex"):
        fc.flip(p, tri, 2)
    with pytest.raises(b.InvalidArgument, match="2 vertices have a coordinate that is not finite"):
        run(ctx, p, tri, 2)
    with pytest.raises(b.InvalidArgument, match="2 vertices have a coordinate that is not finite"):
        run(ctx, p, tri[:0], 2)
    small_correct_call(ctx)
    p, tri = fc.kite()
    for min_gain, min_cos in [(-1e-9, 0.5), (np.inf, 0.5), (np.nan, 0.5), (0.0, 1.5), (0.0, -1.5), (0.0, np.nan)]:
        with pytest.raises(fc.Invalid, match="parameters"):
            fc.flip(p, tri, 1, min_gain, min_cos)
        with pytest.raises(b.InvalidArgument):
            run(ctx, p, tri, 1, min_gain, min_cos)
        small_correct_call(ctx)
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    with pytest.raises(b.InvalidArgument):
        b.check(b.lib().mlsgpu_hip_mesh_flip_edges(ctx.h, one.ptr, 1, one.ptr, 1, 1, 0.0, 0.5, one.ptr, None))     # no stats
    st = b.FlipStats()
    assert 3 * ((2 ** 32 + 2) // 3 - 1) < 2 ** 32 <= 3 * ((2 ** 32 + 2) // 3)
    for num_triangles, num_vertices in ((1, 2 ** 32), ((2 ** 32 + 2) // 3, 10)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_flip_edges(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, 1, 0.0, 0.5, one.ptr,
                                                       C.byref(st)))
    one.free()
    small_correct_call(ctx)


# ---------------------------------------------------------------- the device sink

def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def summed(stats):
    out = dict((name, sum(st[name] for st in stats)) for name in fc.STAT_NAMES if not name.startswith(("minQuality", "quality")))
    out["rounds"] = max(st["rounds"] for st in stats)
    out["converged"] = min(st["converged"] for st in stats)
    for name in ("minQualityBefore", "minQualityAfter"):
        out[name] = min(st[name] for st in stats)
    for name in ("qualityBefore", "qualityAfter"):
        out[name] = [sum(st[name][k] for st in stats) for k in range(16)]
    return out


def seam_edges(chunk, shared):
    """The edges of the chunk between two position rows of `shared`, as pairs of rows."""
    rows = np.ascontiguousarray(chunk["vertices"], np.float32).reshape(-1, 3).view("V12").ravel()
    on = np.array([bytes(r) in shared for r in rows])
    tri = chunk["triangles"].astype(np.int64)
    a, b = tri.ravel(), tri[:, [1, 2, 0]].ravel()
    both = on[a] & on[b]
    return set(frozenset((bytes(rows[x]), bytes(rows[y]))) for x, y in zip(a[both], b[both]))


@pytest.mark.parametrize("chunks", [1, 2])
def test_sink(ctx, tmp_path, chunks):
    """One bucket in one chunk, eight buckets in two: each chunk is the oracle's for its own earlier download, the vertices
    stay, the seam's edges stay, normals and files follow the flipped triangles, a finalize brings the chunks back."""
    import topology_cases as tc
    from mlsgpu_amd import binding as b
    from test_gpu_simplify import CELL, ORIGIN, filled_sink
    from test_gpu_smooth import rows_of
    mesher, buckets = filled_sink(ctx, 47, lambda k: 0) if chunks == 1 else filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    with pytest.raises(b.InvalidArgument):
        mesher.flip_edges(MAX_ROUNDS)                               # before finalize
    assert buckets == (1 if chunks == 1 else 8) and mesher.finalize() == chunks
    before = [mesher.chunk(i) for i in range(chunks)]
    topology = [tc.report_fields(mesher.chunk_topology(i)) for i in range(chunks)]
    shared = rows_of(before[0]["vertices"]) & rows_of(before[-1]["vertices"]) if chunks == 2 else set()
    seams = [seam_edges(c, shared) for c in before]
    assert chunks == 1 or (len(shared) > 100 and all(len(s) > 50 for s in seams))
    mesher.chunk_normals(0)                                         # computed before the call: must not be served after it
    want = [fc.flip(c["vertices"], c["triangles"], MAX_ROUNDS) for c in before]
    st = mesher.flip_edges(MAX_ROUNDS)
    assert st == summed([w[1] for w in want]) and st["converged"] == 1 and st["flips"] > 100
    for i in range(chunks):
        c = mesher.chunk(i)
        assert len(c["triangles"]) > 1000 and c["chunk"] == before[i]["chunk"]
        fc.assert_same((c["triangles"], want[i][1]), want[i])
        assert c["vertices"].tobytes() == before[i]["vertices"].tobytes()
        assert tc.report_fields(mesher.chunk_topology(i)) == topology[i]
        assert seam_edges(c, shared) == seams[i]                    # no seam edge changed
        got = mesher.chunk_normals(i)
        nc.assert_same((got["normals"], got["stats"]), nc.normals(c["vertices"], want[i][0]))
        mesher.write_ply(i, tmp_path / "device.ply", comments=("c",))
        b.write_ply(tmp_path / "host.ply", c["vertices"], want[i][0], comments=("c",))
        assert file_bytes(tmp_path / "device.ply") == file_bytes(tmp_path / "host.ply")
    with pytest.raises(b.InvalidArgument):
        mesher.flip_edges(MAX_ROUNDS, min_cos=2.0)                  # a refused parameter costs no results
    again = mesher.flip_edges(MAX_ROUNDS)                           # it may be called again: a fixed point
    assert (again["flips"], again["rounds"], again["nonDelaunayBefore"]) == (0, 1, st["nonDelaunayAfter"])
    mesher.simplify(ORIGIN, CELL)                                   # and after a simplify
    simplified = [mesher.chunk(i) for i in range(chunks)]
    want = [fc.flip(c["vertices"], c["triangles"], MAX_ROUNDS) for c in simplified]
    assert mesher.flip_edges(MAX_ROUNDS) == summed([w[1] for w in want])
    for i in range(chunks):
        fc.assert_same((mesher.chunk(i)["triangles"], want[i][1]), want[i])
    assert mesher.finalize() == chunks                              # finalize again: the chunks as they were
    for i in range(chunks):
        c = mesher.chunk(i)
        assert c["vertices"].tobytes() == before[i]["vertices"].tobytes() and c["triangles"].tobytes() == before[i]["triangles"].tobytes()
    mesher.close()


# ---------------------------------------------------------------- reconstruct --flip-edges

def test_reconstruct_flip_edges(ctx, tmp_path):
    """examples/reconstruct --flip-edges 64: one more line, and a file that is the oracle's for the file the same command
    writes without the option -- as a mesh over the same positions, since two runs number their vertices in the order their
    worker threads deliver."""
    from test_gpu_normals import same_mesh
    from test_gpu_simplify import shells
    from test_host_cpp import build_example, parse_ply_mesh
    from mlsgpu_amd import synth
    exe = build_example(tmp_path, "reconstruct")
    cloud = shells()
    rows = np.zeros(len(cloud), synth.PLY_ROW)
    rows["p"], rows["n"], rows["r"] = cloud["position"], cloud["normal"], cloud["radius"]
    (tmp_path / "in.ply").write_bytes(synth.ply_header(len(rows)) + rows.tobytes())

    def reconstruct(out, *flags):
        cmd = [exe, "--weld", "device"] + list(flags) + [str(tmp_path / "in.ply"), str(tmp_path / out), "1.0", "1.5", "4", "3", "0.02", "8000"]
        return subprocess.check_output(cmd, timeout=300).decode().splitlines()

    for flags in ((), ("--simplify", "4")):
        plain = reconstruct("plain.ply", *flags)
        out = reconstruct("out.ply", *(flags + ("--flip-edges", "64")))
        assert len(out) == len(plain) + 1 and out[:-1] == plain, out
        V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
        gotV, gotT = parse_ply_mesh(str(tmp_path / "out.ply"))
        want, st = fc.flip(V, tri, 64, 1e-6, 0.5)
        assert len(tri) > 100 and st["flips"] > 10 and same_mesh(gotV, gotT, V, want)
        line = re.fullmatch(r"flip-edges chunks (\d+) interior-edges (\d+) rounds (\d+) flips (\d+) non-delaunay (\d+) -> (\d+) "
                            r"blocked (\d+) min-quality ([-+0-9.e]+) -> ([-+0-9.e]+)", out[-1])
        assert line, out[-1]
        assert [int(x) for x in line.groups()[:7]] == [1, st["interiorEdges"], st["rounds"], st["flips"], st["nonDelaunayBefore"],
                                                       st["nonDelaunayAfter"], st["blockedAfter"]]
        assert [float(x) for x in line.groups()[7:]] == [float("%.9g" % st[name]) for name in ("minQualityBefore", "minQualityAfter")]
    refused = subprocess.run([exe, "--weld", "host", "--flip-edges", "64", str(tmp_path / "in.ply"), str(tmp_path / "host.ply"), "1.0",
                              "1.5", "4", "3", "0.02", "8000"], capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--flip-edges needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
