"""The device vertex normals (mlsgpu_hip_mesh_normals, mlsgpu_hip_mesher_chunk_normals, the PLY writers with normals,
reconstruct --normals) against the CPU oracle of normals_cases.py: normals as uint32 views and all statistics, bit for bit."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import normals_cases as nc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def run(ctx, vertices, triangles):
    from mlsgpu_amd import binding as b
    return b.mesh_normals(ctx, vertices, np.asarray(triangles).astype(np.uint32))


def check(ctx, vertices, triangles):
    want = nc.normals(vertices, triangles)
    nc.assert_same(run(ctx, vertices, triangles), want)
    return want


# ---------------------------------------------------------------- hand case and empty meshes

def test_hand_case_and_empty_meshes(ctx):
    p, tri = nc.grid_mesh(4, 4)
    n, st = run(ctx, p, tri)
    assert n.tolist() == [[0.0, 0.0, 1.0]] * 16
    assert st == dict(numVertices=16, numTriangles=18, outOfRangeTriangles=0, nonFiniteTriangles=0, zeroNormals=0, scaleExponent=0)
    check(ctx, p, tri)
    assert check(ctx, p[:0], tri[:0])[1] == dict.fromkeys(nc.STAT_NAMES, 0)         # V = 0 and T = 0
    assert check(ctx, p, tri[:0])[1]["zeroNormals"] == 16                           # T = 0
    assert check(ctx, p[:0], tri)[1]["outOfRangeTriangles"] == 18                   # V = 0: every index is out of range


# ---------------------------------------------------------------- many workgroups

@pytest.fixture(scope="module")
def big_grid():
    p, tri = nc.grid_mesh(300, 300, jitter=0.3, seed=11)
    assert p.shape == (90_000, 3) and tri.shape == (178_802, 3)
    return p, tri, nc.normals(p, tri)


def test_many_workgroups(ctx, big_grid):
    p, tri, want = big_grid
    nc.assert_same(run(ctx, p, tri), want)
    assert want[1]["zeroNormals"] == 0 and (want[0][:, 2] > 0.5).all()
    assert len(tri[:-1]) % 64 == 49                 # a partial last wave
    check(ctx, p, tri[:-1])


# ---------------------------------------------------------------- contention

def test_fan_around_one_hub(ctx):
    """20 000 triangles whose first corner is vertex 0; then every triangle twice, in a shuffled order, so that the lanes of
    one wave meet the hub and the rim together."""
    p, tri = nc.fan_mesh(20_000, seed=1)
    want = check(ctx, p, tri)
    assert want[1]["zeroNormals"] == 0 and want[0][0, 2] > 0.9
    twice = np.concatenate([tri, tri])[np.random.default_rng(2).permutation(2 * len(tri))]
    doubled = check(ctx, p, twice)
    np.testing.assert_array_equal(doubled[0].view(np.uint32), want[0].view(np.uint32))      # 2 S normalises to the same


# ---------------------------------------------------------------- mixed magnitudes

def test_mixed_magnitudes(ctx):
    """The torus and a copy scaled by 2^-12 as a second component: the small faces are 2^-24 of the large ones and keep seven
    bits of q, and the oracle has to agree on exactly which."""
    p, tri = nc.torus_mesh(400, 60, 0.5, 0.125)
    V = len(p)
    both_p = np.concatenate([p, p * np.float32(2.0 ** -12)])
    both_t = np.concatenate([tri, tri + V])
    n, st = check(ctx, both_p, both_t)
    assert st["zeroNormals"] == 0
    dot = (n[V:].astype(np.float64) * nc.torus_normals(400, 60)).sum(axis=1)
    assert 0.9 < dot.min() < 0.99999                # coarse, and still normals


# ---------------------------------------------------------------- counters and guard bands

def test_counters_and_guard_bands(ctx):
    """The counter cases of the CPU file (counted outcomes: an index >= V is compared, never followed), with dOutNormals
    between two guard bands that must stay as they were."""
    from mlsgpu_amd import binding as b
    p, tri = nc.counter_mesh()
    assert (tri == 0xFFFFFFFF).sum() == 1
    want = check(ctx, p, tri)
    assert (want[1]["outOfRangeTriangles"], want[1]["nonFiniteTriangles"]) == (2, 12)
    p[16, 2] = 0.0                                  # without the far vertex that sets the scale
    want = check(ctx, p, tri)
    assert (want[1]["outOfRangeTriangles"], want[1]["nonFiniteTriangles"], want[1]["zeroNormals"]) == (2, 12, 3)
    V, G = len(p), 1024
    band = np.full(2 * G + 3 * V, -123.25, np.float32)
    dv, dt = b.DeviceBuffer(ctx, array=p), b.DeviceBuffer(ctx, array=tri.astype(np.uint32))
    out = b.DeviceBuffer(ctx, array=band)
    st = b.NormalsStats()
    b.check(b.lib().mlsgpu_hip_mesh_normals(ctx.h, dv.ptr, V, dt.ptr, len(tri), out.ptr + 4 * G, C.byref(st)))
    got = out.download(np.float32)
    for buf in (dv, dt, out):
        buf.free()
    assert (got[:G] == -123.25).all() and (got[G + 3 * V:] == -123.25).all()
    nc.assert_same((got[G:G + 3 * V], st.as_dict()), want)


# ---------------------------------------------------------------- determinism

def test_determinism(ctx, big_grid, monkeypatch):
    p, tri, want = big_grid
    a, b = run(ctx, p, tri), run(ctx, p, tri)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    nc.assert_same(run(ctx, p, tri[np.random.default_rng(3).permutation(len(tri))]), want)
    fan = nc.fan_mesh(20_000, seed=1)
    for mode in ("plain", "wave"):                  # the two accumulate kernels
        monkeypatch.setenv("MLSGPU_HIP_NORMALS_ACCUMULATE", mode)
        nc.assert_same(run(ctx, p, tri), want)
        check(ctx, *fan)


# ---------------------------------------------------------------- errors

def test_length_error_leaves_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st = b.NormalsStats()
    for num_triangles, num_vertices in ((1, 2 ** 32), ((2 ** 32 + 2) // 3, 10)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_normals(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, one.ptr, C.byref(st)))
    one.free()
    check(ctx, *nc.grid_mesh(9, 11, jitter=0.2, seed=3))


# ---------------------------------------------------------------- the device sink

def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_sink_two_chunks(ctx, tmp_path):
    """Eight buckets in two chunks: each chunk's normals are the oracle's for its own download, served again from the same
    place, written as the host writer writes them, and recomputed after a simplify; the plain writer's file does not change."""
    from mlsgpu_amd import binding as b
    from test_gpu_simplify import CELL, ORIGIN, filled_sink
    mesher, buckets = filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    with pytest.raises(b.InvalidArgument):
        mesher.chunk_normals(0)                     # before finalize
    assert buckets == 8 and mesher.finalize() == 2
    plain = []
    for i in range(2):
        mesher.write_ply(i, tmp_path / "plain.ply", comments=("c",))
        plain.append(file_bytes(tmp_path / "plain.ply"))
    for i in range(2):
        c = mesher.chunk(i)
        assert len(c["triangles"]) > 1000
        want = nc.normals(c["vertices"], c["triangles"])
        got = b.mesher_chunk_normals(mesher, i)
        nc.assert_same((got["normals"], got["stats"]), want)
        again = mesher.chunk_normals(i)
        assert again["d_normals"] == got["d_normals"] and again["stats"] == got["stats"]
        assert again["normals"].tobytes() == got["normals"].tobytes()
        # a small buffer: the vertex rows and the faces each travel in several pieces
        b.mesher_write_ply_normals(mesher, i, tmp_path / "device.ply", comments=("c",), buffer_bytes=2 * 312 * 40)
        b.write_ply_normals(tmp_path / "host.ply", c["vertices"], want[0], c["triangles"], comments=("c",))
        assert file_bytes(tmp_path / "device.ply") == file_bytes(tmp_path / "host.ply")
        mesher.write_ply(i, tmp_path / "plain.ply", comments=("c",))
        assert file_bytes(tmp_path / "plain.ply") == plain[i]
    st = mesher.simplify(ORIGIN, CELL)
    assert 0 < st["outTriangles"] < st["inTriangles"]
    for i in range(2):
        c = mesher.chunk(i)
        want = nc.normals(c["vertices"], c["triangles"])
        mesher.write_ply_normals(i, tmp_path / "device.ply")            # computes the chunk's normals itself
        b.write_ply_normals(tmp_path / "host.ply", c["vertices"], want[0], c["triangles"])
        assert file_bytes(tmp_path / "device.ply") == file_bytes(tmp_path / "host.ply")
        got = mesher.chunk_normals(i)
        nc.assert_same((got["normals"], got["stats"]), want)
    assert mesher.finalize() == 2                   # finalize invalidates: the unsimplified chunks again
    c = mesher.chunk(1)
    got = mesher.chunk_normals(1)
    nc.assert_same((got["normals"], got["stats"]), nc.normals(c["vertices"], c["triangles"]))
    mesher.close()


# ---------------------------------------------------------------- reconstruct --normals

def parse_ply_with_normals(path):
    raw = file_bytes(path)
    head_end = raw.index(b"end_header\n") + 11
    head = raw[:head_end].decode("ascii").split("\n")
    props = [l.split()[2] for l in head if l.startswith("property float32")]
    assert props == ["x", "y", "z", "nx", "ny", "nz"], props
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[2])
    nt = int([l for l in head if l.startswith("element face")][0].split()[2])
    rows = np.frombuffer(raw, "<f4", 6 * nv, head_end).reshape(nv, 6)
    faces = np.frombuffer(raw, np.dtype([("n", np.uint8), ("i", "<u4", 3)]), nt, head_end + 24 * nv)
    assert (faces["n"] == 3).all() and head_end + 24 * nv + 13 * nt == len(raw)
    return rows[:, :3], rows[:, 3:], faces["i"]


def same_mesh(va, ta, vb, tb):
    """Two runs of reconstruct weld their bins in the order its worker threads deliver them: the same mesh, its vertices and
    triangles in another order.  Equal here = the same set of positions, and the same triangles over them (as rotations)."""
    import simplify_cases as sc
    rows_a, id_a = np.unique(np.ascontiguousarray(va).view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    rows_b, id_b = np.unique(np.ascontiguousarray(vb).view(np.uint32).reshape(-1, 3), axis=0, return_inverse=True)
    return (len(va) == len(vb) and rows_a.tobytes() == rows_b.tobytes()
            and sc.canonical(id_a.ravel()[np.asarray(ta, np.int64)]) == sc.canonical(id_b.ravel()[np.asarray(tb, np.int64)]))


def test_reconstruct_normals(ctx, tmp_path):
    """examples/reconstruct --normals: the mesh of the run without the flag, the oracle's normals on the file's own arrays,
    one line per chunk with the counters; after --simplify when both are given; refused for the host welder."""
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
        out = reconstruct("out.ply", *(flags + ("--normals",)))
        assert len(out) == len(plain) + 1 and out[:-1] == plain, out
        V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
        gotV, gotN, gotT = parse_ply_with_normals(str(tmp_path / "out.ply"))
        assert same_mesh(gotV, gotT, V, tri) and len(tri) > 100
        want = nc.normals(gotV, gotT)
        np.testing.assert_array_equal(gotN.view(np.uint32), want[0].view(np.uint32))
        line = re.fullmatch(r"normals chunk (\d+) vertices (\d+) zero (\d+) out-of-range (\d+) non-finite (\d+) exponent (-?\d+)", out[-1])
        assert line, out[-1]
        st = want[1]
        assert [int(x) for x in line.groups()[1:]] == [st["numVertices"], st["zeroNormals"], st["outOfRangeTriangles"],
                                                       st["nonFiniteTriangles"], st["scaleExponent"]]
    refused = subprocess.run([exe, "--weld", "host", "--normals", str(tmp_path / "in.ply"), str(tmp_path / "host.ply"), "1.0", "1.5",
                              "4", "3", "0.02", "8000"], capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--normals needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()


# ---------------------------------------------------------------- orientation

def test_normals_point_out_of_the_surface(ctx):
    """Splats on a sphere with radial normals, through a worker into a sink: the field is negative inside, the surface closes
    with positive signed volume, and every vertex normal points away from the centre.  A sign: no tolerance."""
    import mlsgpu_amd as m
    from mlsgpu_amd import synth
    rng = np.random.default_rng(9)
    centre, radius, count = np.array([23.5, 23.5, 23.5]), 16.0, 20_000
    d = rng.normal(size=(count, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    cloud = np.zeros(count, synth.SPLAT_DTYPE)
    cloud["normal"] = d.astype(np.float32)
    cloud["position"] = (centre + radius * d).astype(np.float32)
    cloud["radius"] = rng.uniform(1.5, 2.5, count).astype(np.float32)
    cloud["quality"] = (1.0 / cloud["radius"].astype(np.float64) ** 2).astype(np.float32)
    allb, buckets = synth.bucketize(cloud, 48, 47)
    assert len(buckets) == 1
    dev = m.DeviceBuffer(ctx, array=allb)
    worker = m.Worker(ctx, buckets[0].count, max_cells=63)
    mesher = m.Mesher(ctx, 0.02)
    worker.process(dev, buckets[0].first, buckets[0].count, buckets[0].low, buckets[0].num_vertices, collector=mesher.collector(ctx, 0))
    del worker
    dev.free()
    assert mesher.finalize() == 1
    c = mesher.chunk(0)
    got = mesher.chunk_normals(0)
    nc.assert_same((got["normals"], got["stats"]), nc.normals(c["vertices"], c["triangles"]))
    n, p = got["normals"].astype(np.float64), c["vertices"].astype(np.float64)
    has = np.abs(n).sum(axis=1) > 0
    assert has.sum() > 5000
    assert ((n[has] * (p[has] - centre)).sum(axis=1) > 0).all()
    mesher.close()
