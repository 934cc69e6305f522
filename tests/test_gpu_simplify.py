"""The device simplifier (mlsgpu_hip_mesh_simplify, mlsgpu_hip_mesher_simplify, reconstruct --simplify) against the CPU
oracle of simplify_cases.py: vertices as uint32 views, triangles and all six statistics, bit for bit."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import simplify_cases as sc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def run(ctx, vertices, triangles, origin, cell_size):
    from mlsgpu_amd import binding as b
    return b.mesh_simplify(ctx, vertices, np.asarray(triangles).astype(np.uint32), origin, cell_size)


def check(ctx, vertices, triangles, origin, cell_size):
    got = run(ctx, vertices, triangles, origin, cell_size)
    want = sc.simplify(vertices, triangles, origin, cell_size)
    sc.assert_same(got, want)
    return want


# ---------------------------------------------------------------- hand case and empty meshes

def test_hand_case_and_empty_meshes(ctx):
    p, tri = sc.grid_mesh(4, 4)
    v, t, st = run(ctx, p, tri, (-0.5, -0.5, -0.5), 2.0)
    assert v.tolist() == [[0.5, 0.5, 0.0], [2.5, 0.5, 0.0], [0.5, 2.5, 0.0], [2.5, 2.5, 0.0]]
    assert t.tolist() == [[0, 1, 3], [0, 3, 2]]
    assert st == dict(inVertices=16, inTriangles=18, outVertices=4, outTriangles=2, collapsedTriangles=16, duplicateTriangles=0)
    check(ctx, p, tri, (-0.5, -0.5, -0.5), 2.0)
    check(ctx, p[:0], tri[:0], (-0.5, -0.5, -0.5), 2.0)         # V = 0
    check(ctx, p, tri[:0], (-0.5, -0.5, -0.5), 2.0)             # T = 0


# ---------------------------------------------------------------- several sort tiles

@pytest.fixture(scope="module")
def big_grid():
    p, tri = sc.grid_mesh(300, 300, jitter=0.3, seed=11)
    assert p.shape == (90_000, 3) and tri.shape == (178_802, 3)
    return p, tri


@pytest.mark.parametrize("cell", [0.5, 3.0, 37.5])
def test_several_sort_tiles(ctx, big_grid, cell):
    p, tri = big_grid
    want = check(ctx, p, tri, (-1.0, -1.0, -1.0), cell)[2]
    if cell == 0.5:
        assert want["outTriangles"] > 150_000               # nearly lossless: the triangle sorts span several tiles
    if cell == 37.5:
        assert want["inVertices"] / 81 > 1000 and want["outVertices"] <= 81     # clusters of > 1 000 members


def test_beyond_the_one_launch_scans(ctx):
    """2 102 500 vertices and 4 199 202 triangles: more than the 1 024 tiles of 2 048 elements a scan takes in one launch, so
    all four scans run in their two-launch form (which evaluates its input functor twice, and numbers the used clusters in
    place of their marks)."""
    p, tri = sc.grid_mesh(1450, 1450, jitter=0.3, seed=2)
    assert len(p) > 1024 * 2048 and len(tri) > 1024 * 2048
    want = check(ctx, p, tri, (-1.0, -1.0, -1.0), 3.0)[2]
    assert want["duplicateTriangles"] > 0 and want["outTriangles"] > 500_000


# ---------------------------------------------------------------- cluster sums

def test_cluster_sums(ctx):
    """Coordinates between -1e4 and -8e3 with the origin at -1e4 and a cell of 1e-2: cells up to 2 * 10^5, where the f32
    division rounds by up to 2^-8 of a cell -- the float32 cells differ from exact arithmetic's for some vertices, whose
    offset inside the cell is then negative, and the double fixed-point path has to carry that."""
    p, tri = sc.torus_mesh(400, 60, 0.5, 0.125, (-9000.0, -8000.0, -9500.0))
    origin, cell = (-1.0e4, -1.0e4, -1.0e4), 1.0e-2
    want = check(ctx, p, tri, origin, cell)[2]
    assert 1000 < want["outVertices"] < want["inVertices"] - 1000 and want["collapsedTriangles"] > 1000
    exact = np.floor((p.astype(np.float64) - np.float64(np.float32(origin[0]))) / np.float64(np.float32(cell)))
    assert (exact != sc.cells(p, origin, cell)).sum() > 100


def test_thin_torus_duplicates(ctx):
    p, tri = sc.torus_mesh(97, 6, 10.0, 0.1, windings=2)
    assert check(ctx, p, tri, (-12.5, -12.5, -12.5), 2.5)[2]["duplicateTriangles"] > 0


# ---------------------------------------------------------------- one cluster

def test_one_cluster(ctx):
    p, tri = sc.grid_mesh(100, 200, jitter=0.3, seed=5)
    assert len(p) == 20_000
    want = check(ctx, p, tri, (-1.0, -1.0, -1.0), 1000.0)[2]
    assert (want["outVertices"], want["outTriangles"], want["collapsedTriangles"]) == (0, 0, len(tri))


# ---------------------------------------------------------------- errors

def test_errors_leave_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    p, tri = sc.grid_mesh(9, 11)
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

    cases = [(moved(50, 1, np.nan), tri, origin, 1.0),              # a NaN vertex
             (moved(50, 2, np.inf), tri, origin, 1.0),
             (moved(7, 0, -1.5), tri, origin, 1.0),                 # a vertex below the origin
             (moved(98, 1, 2.0 ** 21 - 1), tri, origin, 1.0),       # a cell at 2^21
             (p, with_index(V), origin, 1.0),                       # an index = V
             (p, with_index(0xFFFFFFFF), origin, 1.0),
             (p, tri, origin, 0.0), (p, tri, origin, -2.0), (p, tri, origin, np.inf), (p, tri, origin, np.nan),
             (p, tri, (np.nan, 0.0, 0.0), 1.0)]
    for args in cases:
        with pytest.raises(sc.Invalid):
            sc.simplify(*args)
        with pytest.raises(b.InvalidArgument):
            run(ctx, *args)
        check(ctx, p, tri, origin, 3.0)                             # the context is still usable
    check(ctx, moved(98, 1, 2.0 ** 21 - 2), tri, origin, 1.0)       # the last cell is fine
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st, frame = b.SimplifyStats(), (C.c_float * 3)(*origin)
    for num_triangles, num_vertices in (((2 ** 32 + 2) // 3, 10), (1, 2 ** 32)):
        with pytest.raises(b.LengthError):                          # refused before any launch: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_simplify(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, frame, 1.0, one.ptr,
                                                     one.ptr, C.byref(st)))
    one.free()


# ---------------------------------------------------------------- determinism

def test_determinism(ctx, big_grid):
    p, tri = big_grid
    a = run(ctx, p, tri, (-1.0, -1.0, -1.0), 3.0)
    b = run(ctx, p, tri, (-1.0, -1.0, -1.0), 3.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


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
    """One bucket through a worker into the device sink; the simplified chunk is the oracle's for the chunk as it was,
    serves the topology report and the PLY writer, and the call may be repeated."""
    import topology_cases as tc
    from mlsgpu_amd import binding as b
    mesher, buckets = filled_sink(ctx, 47, lambda k: 0)
    assert buckets == 1
    with pytest.raises(b.InvalidArgument):
        mesher.simplify(ORIGIN, CELL)                           # before finalize
    assert mesher.finalize() == 1
    before = mesher.chunk(0)
    finalize_stats = mesher.stats()
    want = sc.simplify(before["vertices"], before["triangles"], ORIGIN, CELL)
    assert len(before["triangles"]) > 1000 and want[2]["outTriangles"] < want[2]["inTriangles"] / 4
    st = mesher.simplify(ORIGIN, CELL)
    after = mesher.chunk(0)
    sc.assert_same((after["vertices"], after["triangles"], st), want)
    assert (after["num_vertices"], after["num_triangles"], after["chunk"]) == (st["outVertices"], st["outTriangles"], before["chunk"])
    assert mesher.stats() == finalize_stats
    r = tc.report_fields(mesher.chunk_topology(0))
    assert (r["numVertices"], r["numTriangles"]) == (st["outVertices"], st["outTriangles"])
    assert r == tc.count_all(st["outVertices"], after["triangles"])
    mesher.write_ply(0, tmp_path / "device.ply", comments=("simplified",))
    b.write_ply(tmp_path / "host.ply", after["vertices"], after["triangles"], comments=("simplified",))
    assert (tmp_path / "device.ply").read_bytes() == (tmp_path / "host.ply").read_bytes()
    again = sc.simplify(after["vertices"], after["triangles"], ORIGIN, 2 * CELL)
    st = mesher.simplify(ORIGIN, 2 * CELL)                      # it may be called again
    twice = mesher.chunk(0)
    sc.assert_same((twice["vertices"], twice["triangles"], st), again)
    mesher.close()


def test_sink_two_chunks(ctx):
    """Eight buckets in two chunks: each chunk is the oracle's for its own download, the statistics are the sums."""
    mesher, buckets = filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    assert buckets == 8 and mesher.finalize() == 2
    before = [mesher.chunk(i) for i in range(2)]
    assert [c["chunk"] for c in before] == [7, 3]
    want = [sc.simplify(c["vertices"], c["triangles"], ORIGIN, CELL) for c in before]
    st = mesher.simplify(ORIGIN, CELL)
    for i in range(2):
        after = mesher.chunk(i)
        assert after["chunk"] == before[i]["chunk"]
        sc.assert_same((after["vertices"], after["triangles"], want[i][2]), want[i])
    assert st == dict((name, want[0][2][name] + want[1][2][name]) for name in sc.STAT_NAMES)
    mesher.close()


# ---------------------------------------------------------------- reconstruct --simplify

def test_reconstruct_simplify(ctx, tmp_path):
    """examples/reconstruct --simplify 4: the statistics line, and a file that is the oracle's for the file the same command
    writes without the option."""
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
    out = subprocess.check_output([exe, "--weld", "device", "--simplify", "4"] + args("out.ply"), timeout=300).decode().splitlines()
    assert len(out) == 2 and out[0] == plain[0], out
    number = r"([-+0-9.e]+)"
    line = re.fullmatch(r"simplify cell %s origin %s %s %s vertices (\d+) -> (\d+) triangles (\d+) -> (\d+) collapsed (\d+) "
                        r"duplicate (\d+)" % ((number,) * 4), out[1])
    assert line, out[1]
    cell = float(line.group(1))
    origin = [float(line.group(k)) for k in (2, 3, 4)]
    counts = [int(line.group(k)) for k in range(5, 11)]
    # cellSize = 4 x spacing, origin = the bounding grid's low corner (reference 0 + spacing x its low extent) - one cell
    low = [int(x) for x in re.search(r"grid (-?\d+)\.\.-?\d+ (-?\d+)\.\.-?\d+ (-?\d+)\.\.-?\d+", out[0]).groups()]
    assert cell == 4.0 and origin == [float(np.float32(x) - np.float32(4.0)) for x in low]
    V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
    want = sc.simplify(V, tri, origin, cell)
    assert counts == [len(V), want[2]["outVertices"], len(tri), want[2]["outTriangles"], want[2]["collapsedTriangles"],
                      want[2]["duplicateTriangles"]]
    gotV, gotT = parse_ply_mesh(str(tmp_path / "out.ply"))
    assert (len(gotV), len(gotT)) == (counts[1], counts[3])
    sc.assert_same((gotV, gotT, want[2]), want)
    refused = subprocess.run([exe, "--weld", "host", "--simplify", "4"] + args("host.ply"), capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--simplify needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
