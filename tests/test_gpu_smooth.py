"""The device smoothing (mlsgpu_hip_mesh_smooth, mlsgpu_hip_mesher_smooth, reconstruct --smooth) against the CPU oracle of
smooth_cases.py: positions as uint32 views and every statistic, bit for bit."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import normals_cases as nc
import smooth_cases as sc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

LAM, MU = 0.5, -0.53


def run(ctx, vertices, triangles, iterations, lam=LAM, mu=MU, boundary=sc.FIXED, **kw):
    from mlsgpu_amd import binding as b
    return b.mesh_smooth(ctx, vertices, np.asarray(triangles).astype(np.uint32), iterations, lam, mu, boundary, **kw)


def check(ctx, vertices, triangles, iterations, lam=LAM, mu=MU, boundary=sc.FIXED):
    want = sc.smooth(vertices, triangles, iterations, lam, mu, boundary)
    sc.assert_same(run(ctx, vertices, triangles, iterations, lam, mu, boundary), want)
    return want


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- hand cases and empty meshes

def test_hand_cases_and_empty_meshes(ctx):
    p, tri = sc.octahedron()
    out, st = run(ctx, p, tri, 1, 0.5, -0.5)
    assert out.tolist() == (p * 0.75).tolist()
    assert st == dict(numVertices=6, numTriangles=8, outOfRangeTriangles=0, degenerateTriangles=0, numEdges=12, boundaryEdges=0,
                      boundaryVertices=0, isolatedVertices=0, passes=2, scaleExponent=0, maxMove=0.25, maxCoordinate=1.0)
    check(ctx, p, tri, 1, 0.5, -0.5)
    check(ctx, p, tri, 1, 1.0, 0.0)                                 # mu = 0: the lambda pass alone
    p, tri = sc.grid_mesh(4, 4)
    out, st = run(ctx, p, tri, 3)
    assert out.tobytes() == p.tobytes() and (st["numEdges"], st["boundaryEdges"], st["boundaryVertices"], st["maxMove"]) == (33, 12, 12, 0.0)
    check(ctx, p, tri, 3)
    assert check(ctx, p, tri, 3, boundary=sc.CURVE)[1]["maxMove"] > 0.1
    assert check(ctx, p, tri, 0)[1]["numEdges"] == 33               # no iterations: a copy, the counts filled
    assert check(ctx, p[:0], tri[:0], 2)[1] == dict(dict.fromkeys(sc.STAT_NAMES, 0), passes=4, maxMove=0.0, maxCoordinate=0.0)
    out, st = check(ctx, p, tri[:0], 2)                             # T = 0
    assert st["isolatedVertices"] == 16 and out.tobytes() == p.tobytes()
    assert check(ctx, p[:0], tri, 2)[1]["outOfRangeTriangles"] == 18                # V = 0: every index is out of range
    zeros = np.zeros((16, 3), np.float32)
    zeros[3, 1] = -0.0
    assert check(ctx, zeros, tri, 2, boundary=sc.CURVE)[0].tobytes() == zeros.tobytes()     # M = 0: the input's bits


def test_classification_order(ctx):
    """The hand case that the topology report classifies differently: here an index >= V wins over a vertex twice."""
    import topology_cases as tc
    p, tri = tc.classification_trap()
    for mode in (sc.FIXED, sc.CURVE):
        st = check(ctx, p, tri, 2, boundary=mode)[1]
        assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["numEdges"], st["boundaryEdges"]) == (2, 1, 5, 4)


# ---------------------------------------------------------------- many workgroups

@pytest.fixture(scope="module")
def big_grid():
    p, tri = sc.grid_mesh(300, 300, jitter=0.3, seed=11)
    assert p.shape == (90_000, 3) and tri.shape == (178_802, 3)
    return p, tri, {mode: sc.smooth(p, tri, 3, LAM, MU, mode) for mode in (sc.FIXED, sc.CURVE)}


@pytest.mark.parametrize("mode", [sc.FIXED, sc.CURVE])
def test_several_sort_tiles(ctx, big_grid, mode):
    p, tri, want = big_grid
    sc.assert_same(run(ctx, p, tri, 3, boundary=mode), want[mode])
    assert want[mode][1]["boundaryVertices"] == 4 * 299 and want[mode][1]["maxMove"] > 0.1
    assert 6 * len(tri[:-1]) % 64 != 0 and len(p) % 64 != 0         # a partial last wave of records and of vertices
    check(ctx, p, tri[:-1], 3, boundary=mode)


def test_beyond_the_one_launch_scans(ctx):
    """717 602 triangles: 3 T = 2 152 806 records (and the 6 T this implementation scans) are more than the 1 024 tiles of
    2 048 elements a scan takes in one launch, so the adjacency scan runs in its two-launch form, which evaluates its input
    functor twice."""
    p, tri = sc.grid_mesh(600, 600, jitter=0.3, seed=2)
    assert 3 * len(tri) == 2_152_806 > 1024 * 2048
    assert check(ctx, p, tri, 2)[1]["numEdges"] == 1_077_601


# ---------------------------------------------------------------- a long neighbour list

@pytest.mark.parametrize("mode", [sc.FIXED, sc.CURVE])
def test_fan_around_one_hub(ctx, mode):
    """One interior hub of valence 20 000 and 20 000 boundary vertices; then every triangle twice, in a shuffled order: no
    side is used exactly once, so nothing is on the boundary."""
    p, tri = nc.fan_mesh(20_000, seed=1)
    _, st = check(ctx, p, tri, 2, boundary=mode)
    assert (st["numEdges"], st["boundaryEdges"], st["boundaryVertices"]) == (40_000, 20_000, 20_000) and st["maxMove"] > 0
    twice = np.concatenate([tri, tri])[np.random.default_rng(2).permutation(2 * len(tri))]
    _, st = check(ctx, p, twice, 2, boundary=mode)
    assert (st["numEdges"], st["boundaryEdges"], st["boundaryVertices"]) == (40_000, 0, 0)


# ---------------------------------------------------------------- closed surfaces, far from the origin, scaled

def test_closed_torus_and_scaling(ctx):
    p, tri = sc.noisy_torus(200, 40, 0.004, 7)
    out, st = check(ctx, p, tri, 10)
    assert (st["boundaryVertices"], st["numEdges"], st["scaleExponent"]) == (0, 24_000, -1)
    d = sc.torus_distance(out)
    assert np.sqrt((d * d).mean()) < 0.002 and abs(d.mean()) < 0.001
    far, _ = sc.noisy_torus(200, 40, 0.004, 7, centre=(1000.0, 1000.0, 1000.0))
    assert check(ctx, far, tri, 10)[1]["scaleExponent"] == 9
    for shift in (-7, 40, -100):
        s = np.float32(2.0) ** np.float32(shift)
        scaled, sst = run(ctx, p * s, tri, 10)
        np.testing.assert_array_equal(bits(scaled), bits(out * s))
        assert sst["scaleExponent"] == st["scaleExponent"] + shift and sst["maxMove"] == st["maxMove"] * 2.0 ** shift


# ---------------------------------------------------------------- counters, guard bands, aliasing

def defect_mesh():
    """A jittered grid with a triangle that names vertex 0xFFFFFFFF, one that names V, two degenerate triangles and two
    unused vertices."""
    p, tri = sc.grid_mesh(9, 11, jitter=0.2, seed=3)
    p = np.concatenate([p, [[4.0, 4.0, 1.0], [-2.0, 0.5, 0.25]]]).astype(np.float32)
    tri = tri.copy()
    tri[5, 2] = len(p)
    tri[77, 0] = 0xFFFFFFFF
    tri[20, 1] = tri[20, 0]
    tri[121, 2] = tri[121, 1]
    return p, tri


def test_counters_guard_bands_and_in_place(ctx):
    from mlsgpu_amd import binding as b
    p, tri = defect_mesh()
    assert (tri == 0xFFFFFFFF).sum() == 1
    for mode in (sc.FIXED, sc.CURVE):
        want = check(ctx, p, tri, 3, boundary=mode)
        assert (want[1]["outOfRangeTriangles"], want[1]["degenerateTriangles"], want[1]["isolatedVertices"]) == (2, 2, 2)
        assert want[1]["boundaryEdges"] > 40                        # the rim, and the holes the four triangles leave
    want = sc.smooth(p, tri, 3, LAM, MU, sc.CURVE)
    V, G = len(p), 1024
    band = np.full(2 * G + 3 * V, -123.25, np.float32)
    dv, dt = b.DeviceBuffer(ctx, array=p), b.DeviceBuffer(ctx, array=tri.astype(np.uint32))
    out = b.DeviceBuffer(ctx, array=band)
    st = b.SmoothStats()
    b.check(b.lib().mlsgpu_hip_mesh_smooth(ctx.h, dv.ptr, V, dt.ptr, len(tri), 3, LAM, MU, sc.CURVE, out.ptr + 4 * G, C.byref(st)))
    got = out.download(np.float32)
    assert (got[:G] == -123.25).all() and (got[G + 3 * V:] == -123.25).all()
    sc.assert_same((got[G:G + 3 * V], st.as_dict()), want)
    assert dv.download(np.float32).tobytes() == p.tobytes()         # the input is left alone ...
    b.check(b.lib().mlsgpu_hip_mesh_smooth(ctx.h, dv.ptr, V, dt.ptr, len(tri), 3, LAM, MU, sc.CURVE, dv.ptr, C.byref(st)))
    sc.assert_same((dv.download(np.float32), st.as_dict()), want)   # ... unless it is the output
    for buf in (dv, dt, out):
        buf.free()
    sc.assert_same(run(ctx, p, tri, 3, boundary=sc.CURVE, in_place=True), want)


# ---------------------------------------------------------------- determinism

@pytest.mark.parametrize("kernel", ["serial", "batched"])
def test_both_pass_kernels(ctx, big_grid, monkeypatch, kernel):
    """MLSGPU_HIP_SMOOTH_PASS: the grid (valences 2 to 6 and lists that end inside a round of four), the hub of valence
    20 000, the defects, a closed torus of valence 6 -- the oracle's bits under either kernel."""
    monkeypatch.setenv("MLSGPU_HIP_SMOOTH_PASS", kernel)
    p, tri, want = big_grid
    for mode in (sc.FIXED, sc.CURVE):
        sc.assert_same(run(ctx, p, tri, 3, boundary=mode), want[mode])
        check(ctx, *nc.fan_mesh(20_000, seed=1), 2, boundary=mode)
        check(ctx, *defect_mesh(), 3, boundary=mode)
    check(ctx, *sc.noisy_torus(200, 40, 0.004, 7), 4)
    check(ctx, *sc.octahedron(), 1, 0.5, -0.5)


@pytest.mark.parametrize("mode", [sc.FIXED, sc.CURVE])
def test_determinism(ctx, big_grid, mode):
    p, tri, want = big_grid
    a, b = run(ctx, p, tri, 3, boundary=mode), run(ctx, p, tri, 3, boundary=mode)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    sc.assert_same(run(ctx, p, tri[np.random.default_rng(3).permutation(len(tri))], 3, boundary=mode), want[mode])
    q, qtri, perm = sc.renumbered(p, tri, 4)
    out, st = run(ctx, q, qtri, 3, boundary=mode)
    assert st == want[mode][1]
    np.testing.assert_array_equal(bits(out[perm]), bits(want[mode][0]))


# ---------------------------------------------------------------- errors

def small_correct_call(ctx):
    check(ctx, *sc.grid_mesh(9, 11, jitter=0.2, seed=3), 2, boundary=sc.CURVE)


def test_errors_leave_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    p, tri = nc.counter_mesh()                                      # a vertex at NaN, one at infinity
    with pytest.raises(sc.Invalid, match="vertex"):
        sc.smooth(p, tri, 2, LAM, MU)
    with pytest.raises(b.InvalidArgument, match="2 vertices have a coordinate that is not finite"):
        run(ctx, p, tri, 2)
    small_correct_call(ctx)
    p, tri = sc.octahedron()
    for lam, mu, mode in [(0.0, MU, 0), (1.5, MU, 0), (np.nan, MU, 0), (LAM, 0.1, 0), (LAM, -1.5, 0), (LAM, MU, 7)]:
        with pytest.raises(sc.Invalid, match="parameters"):
            sc.smooth(p, tri, 1, lam, mu, mode)
        with pytest.raises(b.InvalidArgument):
            run(ctx, p, tri, 1, lam, mu, mode)
        small_correct_call(ctx)
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st = b.SmoothStats()
    assert 6 * ((2 ** 32 + 5) // 6 - 1) < 2 ** 32 <= 6 * ((2 ** 32 + 5) // 6)
    for num_triangles, num_vertices in ((1, 2 ** 32), ((2 ** 32 + 5) // 6, 10)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_smooth(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, 1, LAM, MU, 0, one.ptr,
                                                   C.byref(st)))
    one.free()
    small_correct_call(ctx)


def test_divergence(ctx):
    from mlsgpu_amd import binding as b
    p, tri = sc.noisy_torus(40, 12, 0.01, 1)
    _, st = check(ctx, p, tri, 40, 0.3, -1.0)
    assert 2.0e4 < st["maxCoordinate"] < 2.2e4 < 2.0 ** 20
    with pytest.raises(sc.Invalid, match="diverged"):
        sc.smooth(p, tri, 80, 0.3, -1.0)
    with pytest.raises(b.InvalidArgument, match="diverged"):
        run(ctx, p, tri, 80, 0.3, -1.0)
    small_correct_call(ctx)


# ---------------------------------------------------------------- the device sink

def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def summed(stats):
    out = dict((name, sum(st[name] for st in stats)) for name in sc.STAT_NAMES)
    out["passes"] = stats[0]["passes"]
    for name in ("scaleExponent", "maxMove", "maxCoordinate"):
        out[name] = max(st[name] for st in stats)
    return out


def rows_of(vertices):
    return set(map(bytes, np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).view("V12").ravel()))


@pytest.mark.parametrize("chunks", [1, 2])
def test_sink(ctx, tmp_path, chunks):
    """One bucket in one chunk, eight buckets in two: each chunk is the oracle's for its own earlier download, the triangles
    and the topology report stay, normals and files follow the smoothed positions, a finalize brings the chunks back."""
    import topology_cases as tc
    from mlsgpu_amd import binding as b
    from test_gpu_simplify import CELL, ORIGIN, filled_sink
    mesher, buckets = filled_sink(ctx, 47, lambda k: 0) if chunks == 1 else filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    with pytest.raises(b.InvalidArgument):
        mesher.smooth(5)                                            # before finalize
    assert buckets == (1 if chunks == 1 else 8) and mesher.finalize() == chunks
    before = [mesher.chunk(i) for i in range(chunks)]
    topology = [tc.report_fields(mesher.chunk_topology(i)) for i in range(chunks)]
    mesher.chunk_normals(0)                                         # computed before the call: must not be served after it
    want = [sc.smooth(c["vertices"], c["triangles"], 5, LAM, MU) for c in before]
    st = mesher.smooth(5)
    assert st == summed([w[1] for w in want]) and st["passes"] == 10 and st["maxMove"] > 0
    for i in range(chunks):
        c = mesher.chunk(i)
        assert len(c["triangles"]) > 1000 and c["chunk"] == before[i]["chunk"]
        sc.assert_same((c["vertices"], want[i][1]), want[i])
        assert c["triangles"].tobytes() == before[i]["triangles"].tobytes()
        assert tc.report_fields(mesher.chunk_topology(i)) == topology[i]
        got = mesher.chunk_normals(i)
        nc.assert_same((got["normals"], got["stats"]), nc.normals(want[i][0], c["triangles"]))
        mesher.write_ply(i, tmp_path / "device.ply", comments=("c",))
        b.write_ply(tmp_path / "host.ply", want[i][0], c["triangles"], comments=("c",))
        assert file_bytes(tmp_path / "device.ply") == file_bytes(tmp_path / "host.ply")
    with pytest.raises(b.InvalidArgument):
        mesher.smooth(5, lam=0.0)                                   # a refused parameter costs no results
    twice = [sc.smooth(w[0], c["triangles"], 2, LAM, MU, sc.CURVE) for w, c in zip(want, before)]
    assert mesher.smooth(2, boundary=sc.CURVE) == summed([w[1] for w in twice])     # it may be called again
    for i in range(chunks):
        sc.assert_same((mesher.chunk(i)["vertices"], twice[i][1]), twice[i])
    mesher.simplify(ORIGIN, CELL)                                   # and after a simplify
    simplified = [mesher.chunk(i) for i in range(chunks)]
    want = [sc.smooth(c["vertices"], c["triangles"], 5, LAM, MU) for c in simplified]
    assert mesher.smooth(5) == summed([w[1] for w in want])
    for i in range(chunks):
        sc.assert_same((mesher.chunk(i)["vertices"], want[i][1]), want[i])
    assert mesher.finalize() == chunks                              # finalize again: the chunks as they were
    for i in range(chunks):
        c = mesher.chunk(i)
        assert c["vertices"].tobytes() == before[i]["vertices"].tobytes() and c["triangles"].tobytes() == before[i]["triangles"].tobytes()
    mesher.close()


def test_sink_seams_stay_closed(ctx):
    """The position rows that both chunks hold before the call are rows of both afterwards, with the same bits: a vertex two
    chunks share has its fan cut by the split, so it lies on the boundary of each and FIXED holds it."""
    from test_gpu_simplify import filled_sink
    mesher, _ = filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    assert mesher.finalize() == 2
    before = [mesher.chunk(i) for i in range(2)]
    shared = rows_of(before[0]["vertices"]) & rows_of(before[1]["vertices"])
    assert len(shared) > 100
    for c in before:
        on_boundary = sc.adjacency(len(c["vertices"]), c["triangles"])[3]
        held = rows_of(c["vertices"][on_boundary])
        assert shared <= held, "%d shared vertices are not on the chunk's boundary" % len(shared - held)
    assert mesher.smooth(5)["maxMove"] > 0
    for i in range(2):
        assert shared <= rows_of(mesher.chunk(i)["vertices"])
    mesher.close()


# ---------------------------------------------------------------- reconstruct --smooth

def test_reconstruct_smooth(ctx, tmp_path):
    """examples/reconstruct --smooth 5: one more line, and a file that is the oracle's for the file the same command writes
    without the option -- as a set of positions with the triangles over them, since two runs number their vertices in the
    order their worker threads deliver, and renumbering permutes the smoothed positions."""
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
        out = reconstruct("out.ply", *(flags + ("--smooth", "5")))
        assert len(out) == len(plain) + 1 and out[:-1] == plain, out
        V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
        gotV, gotT = parse_ply_mesh(str(tmp_path / "out.ply"))
        want, st = sc.smooth(V, tri, 5, 0.5, -0.53, sc.FIXED)
        assert len(tri) > 100 and st["maxMove"] > 0 and same_mesh(gotV, gotT, want, tri)
        line = re.fullmatch(r"smooth chunks (\d+) vertices (\d+) edges (\d+) boundary-vertices (\d+) isolated (\d+) passes (\d+) "
                            r"max-move ([-+0-9.e]+)", out[-1])
        assert line, out[-1]
        assert [int(x) for x in line.groups()[:6]] == [1, st["numVertices"], st["numEdges"], st["boundaryVertices"],
                                                       st["isolatedVertices"], 10]
        assert float(line.group(7)) == float("%.9g" % st["maxMove"])
    refused = subprocess.run([exe, "--weld", "host", "--smooth", "5", str(tmp_path / "in.ply"), str(tmp_path / "host.ply"), "1.0", "1.5",
                              "4", "3", "0.02", "8000"], capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--smooth needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
