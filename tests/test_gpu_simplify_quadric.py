"""Quadric-error vertex placement on the device (mlsgpu_hip_mesh_simplify_quadric, mlsgpu_hip_mesher_simplify_quadric,
reconstruct --simplify-quadric) against the CPU oracle of simplify_quadric_cases.py: vertices as uint32 views, triangles and
all ten statistics, bit for bit -- and, on every case, the triangles and the six shared statistics against the mean variant on
the same device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import simplify_cases as sc
import simplify_quadric_cases as qc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))


def run(ctx, vertices, triangles, origin, cell_size):
    from mlsgpu_amd import binding as b
    return b.mesh_simplify_quadric(ctx, vertices, np.asarray(triangles).astype(np.uint32), origin, cell_size)


def check(ctx, vertices, triangles, origin, cell_size):
    """The device against the oracle, and against the mean variant on the same device; returns the oracle's result."""
    from mlsgpu_amd import binding as b
    got = run(ctx, vertices, triangles, origin, cell_size)
    want = qc.simplify_quadric(vertices, triangles, origin, cell_size)
    qc.assert_same(got, want)
    mv, mt, mst = b.mesh_simplify(ctx, vertices, np.asarray(triangles).astype(np.uint32), origin, cell_size)
    np.testing.assert_array_equal(got[1], mt)
    assert dict((k, got[2][k]) for k in sc.STAT_NAMES) == mst and mv.shape == got[0].shape
    return want


# ---------------------------------------------------------------- hand cases and empty meshes

def test_hand_cases_and_empty_meshes(ctx):
    p, tri = sc.grid_mesh(4, 4)
    v, t, st = run(ctx, p, tri, (-0.5, -0.5, -0.5), 2.0)
    # a plane: the quadric has rank 1, and the pull towards the mean decides inside the plane
    assert v.tolist() == [[0.5, 0.5, 0.0], [2.5, 0.5, 0.0], [0.5, 2.5, 0.0], [2.5, 2.5, 0.0]]
    assert t.tolist() == [[0, 1, 3], [0, 3, 2]]
    assert st == dict(inVertices=16, inTriangles=18, outVertices=4, outTriangles=2, collapsedTriangles=16, duplicateTriangles=0,
                      solvedVertices=4, flatVertices=0, escapedVertices=0, scaleExponent=-3)
    check(ctx, p, tri, (-0.5, -0.5, -0.5), 2.0)
    check(ctx, p[:0], tri[:0], (-0.5, -0.5, -0.5), 2.0)         # V = 0
    check(ctx, p, tri[:0], (-0.5, -0.5, -0.5), 2.0)             # T = 0
    # a corner of a cube, eight quads per side: three planes meet in the cluster, the vertex goes to the corner
    p, tri = qc.cube_mesh(8, 8.0)
    want = check(ctx, p, tri, (-1.0, -1.0, -1.0), 3.0)
    assert np.abs(want[0][0]).max() < 0.01                       # the mean lies at (2/3, 2/3, 2/3)


# ---------------------------------------------------------------- creases

@pytest.mark.parametrize("cell", [1.6, 3.7])
def test_cube(ctx, cell):
    p, tri = qc.cube_mesh(24, 24.0, 0.3, 0)
    st = check(ctx, p, tri, (-1.3, -2.1, -0.7), cell)[2]
    assert st["solvedVertices"] > 200 and st["escapedVertices"] + st["flatVertices"] == 0


# ---------------------------------------------------------------- several sort tiles, every route of the accumulation

@pytest.fixture(scope="module")
def big_grid():
    p, tri = sc.grid_mesh(300, 300, jitter=0.3, seed=11)
    assert p.shape == (90_000, 3) and tri.shape == (178_802, 3)
    return p, tri


BIG_ORIGIN = (-1.0, -1.0, -1.0)
BIG_CELLS = [0.5, 37.5]     # nearly lossless: lanes that share no cluster; clusters of > 1 000 members: whole waves inside one


@pytest.mark.parametrize("cell", BIG_CELLS + [3.0])
def test_several_sort_tiles(ctx, big_grid, cell):
    p, tri = big_grid
    want = check(ctx, p, tri, BIG_ORIGIN, cell)[2]
    if cell == 0.5:
        assert want["outTriangles"] > 150_000
    if cell == 37.5:
        assert want["inVertices"] / 81 > 1000 and want["outVertices"] <= 81


def child_main(cell, path):
    """In a fresh process: the big grid at `cell` into an .npz."""
    import mlsgpu_amd as m
    p, tri = sc.grid_mesh(300, 300, jitter=0.3, seed=11)
    c = m.Context(0)
    v, t, st = m.mesh_simplify_quadric(c, p, tri.astype(np.uint32), BIG_ORIGIN, cell)
    c.close()
    np.savez(path, v=v, t=t, st=np.array([st[k] for k in qc.STAT_NAMES], np.int64))


@pytest.mark.parametrize("cell", BIG_CELLS)
def test_plain_accumulation_gives_the_same_bits(big_grid, cell, tmp_path):
    """MLSGPU_HIP_SIMPLIFY_ACCUMULATE=plain in a fresh child process: every lane sends its own atomics."""
    p, tri = big_grid
    path = str(tmp_path / "plain.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_simplify_quadric as t; t.child_main(%r, %r)"
            % (TESTS, os.path.dirname(TESTS), cell, path))
    env = dict(os.environ, MLSGPU_HIP_SIMPLIFY_ACCUMULATE="plain")
    done = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], env=env, timeout=120,
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(path)
    want = qc.simplify_quadric(p, tri, BIG_ORIGIN, cell)
    qc.assert_same((got["v"], got["t"], dict(zip(qc.STAT_NAMES, got["st"].tolist()))), want)


# ---------------------------------------------------------------- one cluster

def test_one_cluster(ctx):
    """Every triangle collapses: nothing comes out, and the sums of the one cluster are still taken."""
    p, tri = sc.grid_mesh(100, 200, jitter=0.3, seed=5)
    want = check(ctx, p, tri, (-1.0, -1.0, -1.0), 1000.0)[2]
    assert (want["outVertices"], want["outTriangles"], want["collapsedTriangles"]) == (0, 0, len(tri))
    assert want["solvedVertices"] + want["flatVertices"] + want["escapedVertices"] == 0 and want["scaleExponent"] != 0


# ---------------------------------------------------------------- the fallbacks

def test_wedge_and_flat_clusters(ctx):
    p, tri, origin, cell = qc.wedge_mesh()
    st = check(ctx, p, tri, origin, cell)[2]
    assert st["escapedVertices"] >= 1 and st["solvedVertices"] >= 1
    p, tri = qc.line_mesh()
    from mlsgpu_amd import binding as b
    want = check(ctx, p, tri, (-0.2, 0.0, 0.0), 1.0)
    assert want[2]["flatVertices"] >= 1 and want[2]["scaleExponent"] == 0
    mean = b.mesh_simplify(ctx, p, tri, (-0.2, 0.0, 0.0), 1.0)
    assert mean[0].tobytes() == want[0].tobytes()                # every cluster falls back: the mean variant's bits
    p, tri = qc.flat_and_grid_mesh()
    st = check(ctx, p, tri, (-0.2, -1.0, 0.0), 1.0)[2]
    assert st["flatVertices"] >= 1 and st["solvedVertices"] >= 1


def test_thin_torus_duplicates(ctx):
    p, tri = sc.torus_mesh(97, 6, 10.0, 0.1, windings=2)
    assert check(ctx, p, tri, (-12.5, -12.5, -12.5), 2.5)[2]["duplicateTriangles"] > 0


def test_far_cells(ctx):
    """Cells up to 2 * 10^5, where the float32 cell of some vertices is not exact arithmetic's: their centred offset leaves
    [-0.5, 0.5], and d and the sums have to carry that."""
    p, tri = sc.torus_mesh(400, 60, 0.5, 0.125, (-9000.0, -8000.0, -9500.0))
    st = check(ctx, p, tri, (-1.0e4, -1.0e4, -1.0e4), 1.0e-2)[2]
    assert st["solvedVertices"] > 1000


# ---------------------------------------------------------------- determinism

def test_determinism(ctx, big_grid):
    p, tri = big_grid
    a = run(ctx, p, tri, BIG_ORIGIN, 3.0)
    b = run(ctx, p, tri, BIG_ORIGIN, 3.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    qc.assert_same(run(ctx, p, qc.permuted_triangles(tri, 3), BIG_ORIGIN, 3.0), a)


# ---------------------------------------------------------------- errors

def test_errors_leave_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    p, tri = sc.grid_mesh(9, 11, jitter=0.2, seed=8)
    V = len(p)
    origin = (-1.0, -1.0, -1.0)

    def moved(index, axis, value):
        q = p.copy()
        q[index, axis] = value
        return q

    def with_index(value):
        t = tri.copy()
        t[40, 1] = value
        return t

    cases = [(p, with_index(V), origin, 1.0), (p, with_index(0xFFFFFFFF), origin, 1.0),       # a bad index
             (moved(50, 1, np.nan), tri, origin, 1.0), (moved(50, 2, np.inf), tri, origin, 1.0),  # a non-finite vertex
             (moved(98, 1, 2.0 ** 21 - 1), tri, origin, 1.0), (moved(7, 0, -1.5), tri, origin, 1.0),  # beyond the 2^21 cells
             (p, tri, origin, 0.0), (p, tri, origin, -2.0), (p, tri, origin, np.inf), (p, tri, origin, np.nan),
             (p, tri, (np.nan, 0.0, 0.0), 1.0)]
    for args in cases:
        with pytest.raises(sc.Invalid):
            qc.simplify_quadric(*args)
        with pytest.raises(b.InvalidArgument):
            run(ctx, *args)
        check(ctx, p, tri, origin, 3.0)                             # the context is still usable
    check(ctx, moved(98, 1, 2.0 ** 21 - 2), tri, origin, 1.0)       # the last cell is fine
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st, frame = b.SimplifyQuadricStats(), (C.c_float * 3)(*origin)
    for num_triangles, num_vertices in (((2 ** 32 + 2) // 3, 10), (1, 2 ** 32)):
        with pytest.raises(b.LengthError):                          # refused before any launch: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_simplify_quadric(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, frame, 1.0,
                                                             one.ptr, one.ptr, C.byref(st)))
    for null in ("vertices", "triangles"):
        with pytest.raises(b.InvalidArgument):
            b.check(b.lib().mlsgpu_hip_mesh_simplify_quadric(ctx.h, None if null == "vertices" else one.ptr, 1,
                                                             None if null == "triangles" else one.ptr, 1, frame, 1.0, one.ptr,
                                                             one.ptr, C.byref(st)))
    one.free()


# ---------------------------------------------------------------- the device sink

SPLATS, EXTENT = 20_000, 47.0
CELL = 4.0                      # 4 x the grid spacing of 1
ORIGIN = (-CELL, -CELL, -CELL)  # the grid's low corner minus one cell


def shells():
    from mlsgpu_amd import synth
    return synth.shells_cloud(SPLATS, EXTENT, 16.0, 1.5, 2.5, seed=5)       # grid units


def filled_sink(ctx, max_cells, chunk_of):
    """The shells cloud, bucket k into chunk chunk_of(k) of a device sink; not yet finalized."""
    import mlsgpu_amd as m
    from mlsgpu_amd import synth
    allb, buckets = synth.bucketize(shells(), int(EXTENT) + 1, max_cells)
    dev = m.DeviceBuffer(ctx, array=allb)
    worker = m.Worker(ctx, max(bk.count for bk in buckets), max_cells=63)
    mesher = m.Mesher(ctx, 0.02)
    for k, bk in enumerate(buckets):
        worker.process(dev, bk.first, bk.count, bk.low, bk.num_vertices, collector=mesher.collector(ctx, chunk_of(k)))
    del worker
    dev.free()
    return mesher, len(buckets)


def test_sink_output(ctx, tmp_path):
    """One bucket through a worker into the device sink; the simplified chunk is the oracle's for the chunk as it was, serves
    the PLY writer, drops the chunk's normals, and the call may be repeated."""
    from mlsgpu_amd import binding as b
    mesher, buckets = filled_sink(ctx, 47, lambda k: 0)
    assert buckets == 1
    with pytest.raises(b.InvalidArgument):
        mesher.simplify_quadric(ORIGIN, CELL)                   # before finalize
    assert mesher.finalize() == 1
    before = mesher.chunk(0)
    finalize_stats = mesher.stats()
    assert mesher.chunk_normals(0)["stats"]["numVertices"] == before["num_vertices"]
    want = qc.simplify_quadric(before["vertices"], before["triangles"], ORIGIN, CELL)
    assert len(before["triangles"]) > 1000 and want[2]["outTriangles"] < want[2]["inTriangles"] / 4
    assert want[2]["solvedVertices"] > 100
    st = mesher.simplify_quadric(ORIGIN, CELL)
    after = mesher.chunk(0)
    qc.assert_same((after["vertices"], after["triangles"], st), want)
    assert (after["num_vertices"], after["num_triangles"], after["chunk"]) == (st["outVertices"], st["outTriangles"], before["chunk"])
    assert mesher.stats() == finalize_stats
    assert mesher.chunk_normals(0)["stats"]["numVertices"] == st["outVertices"]     # those of the simplified chunk
    mesher.write_ply(0, tmp_path / "device.ply", comments=("simplified",))
    b.write_ply(tmp_path / "host.ply", after["vertices"], after["triangles"], comments=("simplified",))
    assert (tmp_path / "device.ply").read_bytes() == (tmp_path / "host.ply").read_bytes()
    again = qc.simplify_quadric(after["vertices"], after["triangles"], ORIGIN, 2 * CELL)
    st = mesher.simplify_quadric(ORIGIN, 2 * CELL)              # it may be called again
    twice = mesher.chunk(0)
    qc.assert_same((twice["vertices"], twice["triangles"], st), again)
    mesher.close()


def test_sink_two_chunks(ctx):
    """Eight buckets in two chunks: each chunk is the oracle's for its own download, the counts are the sums and the exponent
    is the larger one."""
    mesher, buckets = filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    assert buckets == 8 and mesher.finalize() == 2
    before = [mesher.chunk(i) for i in range(2)]
    assert [c["chunk"] for c in before] == [7, 3]
    want = [qc.simplify_quadric(c["vertices"], c["triangles"], ORIGIN, CELL) for c in before]
    st = mesher.simplify_quadric(ORIGIN, CELL)
    for i in range(2):
        after = mesher.chunk(i)
        assert after["chunk"] == before[i]["chunk"]
        qc.assert_same((after["vertices"], after["triangles"], want[i][2]), want[i])
    assert st == dict([(name, want[0][2][name] + want[1][2][name]) for name in qc.STAT_NAMES[:-1]]
                      + [("scaleExponent", max(want[0][2]["scaleExponent"], want[1][2]["scaleExponent"]))])
    mesher.close()


# ---------------------------------------------------------------- reconstruct --simplify-quadric

def test_reconstruct_simplify_quadric(ctx, tmp_path):
    """examples/reconstruct --simplify-quadric 4: the statistics line, and a file that is the oracle's for the file the same
    command writes without the option."""
    from test_host_cpp import build_example, parse_ply_mesh
    from mlsgpu_amd import synth
    exe = build_example(tmp_path, "reconstruct")
    cloud = shells()
    rows = np.zeros(len(cloud), synth.PLY_ROW)
    rows["p"], rows["n"], rows["r"] = cloud["position"], cloud["normal"], cloud["radius"]
    (tmp_path / "in.ply").write_bytes(synth.ply_header(len(rows)) + rows.tobytes())

    def args(out):
        return [str(tmp_path / "in.ply"), str(tmp_path / out), "1.0", "1.5", "4", "3", "0.02", "8000"]

    plain = subprocess.check_output([exe, "--weld", "device"] + args("plain.ply"), timeout=300).decode().splitlines()
    assert len(plain) == 1
    out = subprocess.check_output([exe, "--weld", "device", "--simplify-quadric", "4"] + args("out.ply"), timeout=300).decode().splitlines()
    assert len(out) == 2 and out[0] == plain[0], out
    number = r"([-+0-9.e]+)"
    line = re.fullmatch(r"simplify-quadric cell %s origin %s %s %s vertices (\d+) -> (\d+) triangles (\d+) -> (\d+) collapsed (\d+) "
                        r"duplicate (\d+) solved (\d+) flat (\d+) escaped (\d+) scale-exponent (-?\d+)" % ((number,) * 4), out[1])
    assert line, out[1]
    cell = float(line.group(1))
    origin = [float(line.group(k)) for k in (2, 3, 4)]
    counts = [int(line.group(k)) for k in range(5, 15)]
    low = [int(x) for x in re.search(r"grid (-?\d+)\.\.-?\d+ (-?\d+)\.\.-?\d+ (-?\d+)\.\.-?\d+", out[0]).groups()]
    assert cell == 4.0 and origin == [float(np.float32(x) - np.float32(4.0)) for x in low]
    V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
    want = qc.simplify_quadric(V, tri, origin, cell)
    ws = want[2]
    assert counts == [len(V), ws["outVertices"], len(tri), ws["outTriangles"], ws["collapsedTriangles"], ws["duplicateTriangles"],
                      ws["solvedVertices"], ws["flatVertices"], ws["escapedVertices"], ws["scaleExponent"]]
    gotV, gotT = parse_ply_mesh(str(tmp_path / "out.ply"))
    qc.assert_same((gotV, gotT, ws), want)
    both = subprocess.run([exe, "--weld", "device", "--simplify", "4", "--simplify-quadric", "4"] + args("both.ply"),
                          capture_output=True, timeout=300)
    assert both.returncode != 0 and b"--simplify and --simplify-quadric exclude each other" in both.stderr
    refused = subprocess.run([exe, "--weld", "host", "--simplify-quadric", "4"] + args("host.ply"), capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--simplify-quadric needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists() and not (tmp_path / "both.ply").exists()
