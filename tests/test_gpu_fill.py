"""mlsgpu_hip_mesh_fill_holes / mlsgpu_hip_mesher_fill_holes on the GPU: every result bit for bit the oracle's (fill_cases.fill)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import fill_cases as fc
import normals_cases as nc
import topology_cases as tc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

ALL = 2 ** 20


def run(ctx, vertices, triangles, max_edges, pinned=None):
    from mlsgpu_amd import binding as b
    return b.mesh_fill_holes(ctx, vertices, np.asarray(triangles).astype(np.uint32), max_edges, pinned)


def check(ctx, vertices, triangles, max_edges, pinned=None):
    want = fc.fill(vertices, triangles, max_edges, pinned)
    fc.assert_same(run(ctx, vertices, triangles, max_edges, pinned), want)
    return want


# ---------------------------------------------------------------- hand cases and empty meshes

def test_hand_cases_and_empty_meshes(ctx):
    p = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 3]], np.float32)
    v, t, st = run(ctx, p, [[0, 1, 2]], 3)                          # a single triangle gets a cap
    assert v.tolist() == p.tolist() + [[1.0, 1.0, 1.0]] and t.tolist() == [[0, 1, 2], [1, 0, 3], [2, 1, 3], [0, 2, 3]]
    assert st == dict(numVertices=3, numTriangles=1, outOfRangeTriangles=0, degenerateTriangles=0, boundaryEdges=3, irregularEdges=0,
                      loops=1, filledLoops=1, longLoops=0, pinnedLoops=0, filledEdges=3, longestLoop=3, outVertices=4,
                      outTriangles=4, scaleExponent=1)
    p, tri = fc.octahedron()
    assert check(ctx, p, tri[1:], 8)[1][7:].tolist() == [[4, 0, 6], [0, 2, 6], [2, 4, 6]]
    assert check(ctx, p, tri, 8)[2]["boundaryEdges"] == 0
    p, tri = fc.torus_mesh(7, 5, 0.5, 0.125)
    assert check(ctx, p, tri, 100)[2]["outTriangles"] == 70         # closed: nothing changes
    p, tri = fc.grid_mesh(4, 4)
    assert not any(check(ctx, p[:0], tri[:0], 3)[2].values())       # V = 0 and T = 0
    assert check(ctx, p[:0], tri, 3)[2]["outOfRangeTriangles"] == 18        # V = 0: every index is out of range, and copied
    assert check(ctx, p, tri[:0], 3)[2]["outVertices"] == 16        # T = 0
    zeros = np.zeros((16, 3), np.float32)
    zeros[3, 1] = -0.0
    v, _, st = check(ctx, zeros, tri, 12)                           # M = 0: e = 0, the cap at zero
    assert st["filledLoops"] == 1 and st["scaleExponent"] == 0 and v[16].tolist() == [0, 0, 0]
    tiny = (p * np.float32(2.0 ** -140)).astype(np.float32)         # subnormal coordinates: e is the true exponent
    assert check(ctx, tiny, tri, 12)[2]["scaleExponent"] == 1 - 140


def test_classification_order(ctx):
    """The hand case that the topology report classifies differently: here an index >= V wins over a vertex twice."""
    p, tri = tc.classification_trap()
    v, t, st = check(ctx, p, tri, 8)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["filledLoops"], st["filledEdges"]) == (2, 1, 1, 4)
    assert t[:5].tolist() == tri.tolist() and v[4].tolist() == [0.5, 0.5, 0.0]


# ---------------------------------------------------------------- many workgroups

HOLES = [(10, 10, 1, 1), (50, 60, 2, 3), (100, 200, 8, 8), (200, 100, 1, 1), (201, 101, 1, 1)]


@pytest.fixture(scope="module")
def big_grid():
    p, tri = fc.punched(300, 300, HOLES, jitter=0.3, seed=11)
    assert p.shape == (90_000, 3) and tri.shape == (178_802 - 2 * (1 + 6 + 64 + 2), 3)
    assert 3 * len(tri) % 64 != 0 and len(p) % 64 != 0 and 3 * len(tri) > 100 * 4096    # partial last waves, many sort tiles
    return p, tri, {n: fc.fill(p, tri, n) for n in (4, 10, 31, 32, ALL)}


@pytest.mark.parametrize("max_edges", [4, 10, 31, 32, ALL])
def test_punched_grid(ctx, big_grid, max_edges):
    """Holes of 4, 10 and 32 sides, a figure of eight (8 irregular sides) and the rim of 1 196: at 2^20 the rim is capped too,
    one root shared by a whole launch."""
    p, tri, want = big_grid
    st = want[max_edges][2]
    filled = [n for n in (4, 10, 32, 1196) if n <= max_edges]
    assert (st["loops"], st["irregularEdges"], st["longestLoop"], st["boundaryEdges"]) == (4, 8, 1196, 4 + 10 + 32 + 8 + 1196)
    assert (st["filledLoops"], st["filledEdges"], st["longLoops"]) == (len(filled), sum(filled), 4 - len(filled))
    fc.assert_same(run(ctx, p, tri, max_edges), want[max_edges])


def test_compacted_and_torus(ctx):
    p, tri = fc.punched(61, 67, [(3, 3, 1, 1), (20, 30, 3, 4), (40, 11, 5, 2)], jitter=0.25, seed=4, compact=True)
    assert check(ctx, p, tri, 14)[2]["filledLoops"] == 3
    assert check(ctx, p, tri, ALL)[2]["filledLoops"] == 4
    p, tri = fc.punched_torus(60, 25, [(1, 1, 1, 1), (30, 10, 3, 2), (50, 20, 1, 3)])
    _, t, st = check(ctx, p, tri, 10)
    assert st["filledLoops"] == 3 and tc.count_all(st["outVertices"], t)["numBoundaries"] == 0


# ---------------------------------------------------------------- defects, pinned vertices, one long loop

def test_defects(ctx):
    p, tri = fc.punched(30, 41, [(5, 5, 1, 1), (12, 20, 2, 2)], jitter=0.2, seed=9)
    bad = tri.copy()
    bad[5, 2] = len(p)
    bad[77, 0] = 0xFFFFFFFF
    bad[20, 1] = bad[20, 0]
    bad[121, 2] = bad[121, 1]
    st = check(ctx, p, bad, 100)[2]
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 2) and st["filledLoops"] >= 2
    twice = np.concatenate([tri, tri])[np.random.default_rng(2).permutation(2 * len(tri))]
    st = check(ctx, p, twice, ALL)[2]                               # every side twice: nothing is boundary
    assert st["boundaryEdges"] == 0 and st["outTriangles"] == 2 * len(tri)
    again = np.concatenate([tri, [[0, 41, len(p) - 1]]])            # the rim's side 0 -> 41 used twice in one direction
    st = check(ctx, p, again, ALL)[2]
    assert st["irregularEdges"] > 0 and st["filledLoops"] == 2
    p, tri = fc.figure_eight(jitter=0.1, seed=1)
    assert check(ctx, p, tri, ALL)[2]["irregularEdges"] == 8


def test_pinned_mask(ctx, big_grid):
    p, tri, want = big_grid
    pinned = np.zeros(len(p), np.uint8)
    pinned[50 * 300 + 60] = 1                                       # a corner of the hole of 10 sides
    pinned[5 * 300 + 5] = 7                                         # an interior vertex: on no boundary side
    _, _, st = check(ctx, p, tri, 32, pinned)
    assert (st["filledLoops"], st["pinnedLoops"], st["longLoops"], st["filledEdges"]) == (2, 1, 1, 36)
    _, _, st = check(ctx, p, tri, 4, pinned)                        # long comes before pinned
    assert (st["filledLoops"], st["pinnedLoops"], st["longLoops"]) == (1, 0, 3)
    every = np.ones(len(p), bool)
    assert check(ctx, p, tri, ALL, every)[2]["pinnedLoops"] == 4


def test_one_long_loop(ctx):
    """nc.fan_mesh: 20 000 rim vertices in one loop, consecutive indices, so every wave of the loops and sums kernels holds 64
    vertices of one root."""
    p, tri = nc.fan_mesh(20_000, seed=1)
    v, t, st = check(ctx, p, tri, ALL)
    assert (st["loops"], st["filledLoops"], st["filledEdges"], st["longestLoop"]) == (1, 1, 20_000, 20_000)
    assert tc.count_all(len(v), t)["numBoundaries"] == 0
    st = check(ctx, p, tri, 64)[2]
    assert (st["loops"], st["filledLoops"], st["longLoops"], st["outTriangles"]) == (1, 0, 1, 20_000)


# ---------------------------------------------------------------- capacities and guard bands

def test_capacities_and_guard_bands(ctx, big_grid):
    from mlsgpu_amd import binding as b
    p, tri, wants = big_grid
    want = wants[32]
    V, T, V2, T2, G = len(p), len(tri), want[2]["outVertices"], want[2]["outTriangles"], 1024
    assert (V2, T2) == (V + 3, T + 46)
    dv, dt = b.DeviceBuffer(ctx, array=p), b.DeviceBuffer(ctx, array=tri.astype(np.uint32))
    band_v, band_t = np.full(2 * G + 3 * V2, -123.25, np.float32), np.full(2 * G + 3 * T2, 0xDEADBEEF, np.uint32)
    ov, ot = b.DeviceBuffer(ctx, array=band_v), b.DeviceBuffer(ctx, array=band_t)

    def call(cap_v, cap_t, with_outputs=True):
        st = b.FillStats()
        rc = b.lib().mlsgpu_hip_mesh_fill_holes(ctx.h, dv.ptr, V, dt.ptr, T, 32, None, ov.ptr + 4 * G if with_outputs else None, cap_v,
                                                ot.ptr + 4 * G if with_outputs else None, cap_t, C.byref(st))
        return rc, st.as_dict()

    def untouched():
        return ov.download(np.float32).tobytes() == band_v.tobytes() and ot.download(np.uint32).tobytes() == band_t.tobytes()

    assert call(0, 0, with_outputs=False) == (2, want[2])           # the size query
    assert b"the filled mesh has" in b.lib().mlsgpu_hip_last_error()
    assert call(V2 - 1, T2) == (2, want[2]) and untouched()         # one short in vertices
    assert call(V2, T2 - 1) == (2, want[2]) and untouched()         # one short in triangles
    rc, st = call(V2, T2)
    assert rc == 0
    got_v, got_t = ov.download(np.float32), ot.download(np.uint32)
    assert (got_v[:G] == -123.25).all() and (got_v[G + 3 * V2:] == -123.25).all()
    assert (got_t[:G] == 0xDEADBEEF).all() and (got_t[G + 3 * T2:] == 0xDEADBEEF).all()
    fc.assert_same((got_v[G:G + 3 * V2], got_t[G:G + 3 * T2], st), want)
    assert dv.download(np.float32).tobytes() == p.tobytes()         # the inputs are left alone
    for buf in (dv, dt, ov, ot):
        buf.free()


# ---------------------------------------------------------------- errors

def small_correct_call(ctx):
    check(ctx, *fc.punched(9, 11, [(3, 4, 2, 2)], jitter=0.2, seed=3), 8)


def test_errors_leave_the_context_usable(ctx):
    import mlsgpu_amd as m
    from mlsgpu_amd import binding as b
    p, tri = fc.punched(9, 11, [(3, 4, 2, 2)], jitter=0.2, seed=3)
    for max_edges in (2, ALL + 1):
        with pytest.raises(fc.Invalid):
            fc.fill(p, tri, max_edges)
        with pytest.raises(b.InvalidArgument):
            run(ctx, p, tri, max_edges)
        small_correct_call(ctx)
    q = p.copy()
    q[7, 2] = np.nan
    q[50, 0] = np.inf
    with pytest.raises(fc.Invalid, match="vertex"):
        fc.fill(q, tri, 8)
    with pytest.raises(b.InvalidArgument, match="2 coordinates are not finite"):
        run(ctx, q, tri, 8)
    small_correct_call(ctx)
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st = b.FillStats()
    for num_triangles, num_vertices in ((1, 2 ** 32), ((2 ** 32 + 2) // 3, 10)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_fill_holes(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, 8, None, None, 0, None, 0,
                                                       C.byref(st)))
    one.free()
    small_correct_call(ctx)
    mesher = m.Mesher(ctx, 0.02)
    with pytest.raises(b.InvalidArgument):
        mesher.fill_holes(8)                                        # before finalize
    mesher.close()
    small_correct_call(ctx)


# ---------------------------------------------------------------- determinism

def test_determinism(ctx, big_grid):
    p, tri, want = big_grid
    runs = [run(ctx, p, tri, ALL) for _ in range(3)]
    for r in runs:
        assert r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes() and r[2] == runs[0][2]
    fc.assert_same(runs[0], want[ALL])
    order = np.random.default_rng(3).permutation(len(tri))          # the order of the triangles moves the copied prefix only
    v, t, st = run(ctx, p, tri[order], ALL)
    assert st == want[ALL][2] and v.tobytes() == want[ALL][0].tobytes() and t[len(tri):].tobytes() == want[ALL][1][len(tri):].tobytes()
    small = fc.punched(40, 40, [(5, 5, 1, 1), (10, 20, 2, 3), (20, 8, 2, 2), (28, 25, 8, 8)], jitter=0.2, seed=3, compact=True)
    soup = fc.soup(*check(ctx, *small, 12)[:2])
    q, qtri, _ = fc.renumbered(*small, 4)
    v, t, st = check(ctx, q, qtri, 12)
    assert st["filledLoops"] == 3 and fc.soup(v, t) == soup


# ---------------------------------------------------------------- beyond the one-launch scan

def test_beyond_the_one_launch_scans(ctx):
    """Both scans here run over the vertices: more than 1 024 tiles of 2 048 take the two-launch form, which evaluates its
    input functor twice.  A small punched grid whose vertices lie around index 2 097 152, among vertices that nothing uses."""
    small, tri = fc.punched(30, 30, [(3, 3, 1, 1), (10, 12, 2, 3), (20, 20, 3, 3)], jitter=0.2, seed=6)
    V, first = 1024 * 2048 + 600, 1024 * 2048 - 450
    rng = np.random.default_rng(8)
    p = rng.uniform(-50, 50, (V, 3)).astype(np.float32)
    p[first:first + len(small)] = small
    assert first < 1024 * 2048 < first + len(small) and V > 1024 * 2048
    _, t, st = check(ctx, p, tri + first, 12)
    assert (st["filledLoops"], st["longLoops"], st["outVertices"]) == (3, 1, V + 3)
    assert t[-1].tolist()[1] > 1024 * 2048 > t[len(tri)].tolist()[1]        # new triangles from both sides of the tile border


# ---------------------------------------------------------------- the device sink

def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def summed(stats):
    out = dict((name, sum(st[name] for st in stats)) for name in fc.STAT_NAMES)
    for name in ("longestLoop", "scaleExponent"):
        out[name] = max(st[name] for st in stats)
    return out


def rows_of(vertices):
    return set(map(bytes, np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).view("V12").ravel()))


def in_rows(vertices, rows):
    """Per vertex: is its position, as 12 bytes, one of `rows`."""
    return np.array([bytes(r) in rows for r in np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).view("V12").ravel()], bool)


def boundary_rows(c):
    fa, fb, _, _ = fc.boundary_sides(len(c["vertices"]), c["triangles"])
    return rows_of(c["vertices"][np.union1d(fa, fb)])


@pytest.mark.parametrize("chunks", [1, 2])
def test_sink(ctx, tmp_path, chunks):
    """One bucket in one chunk, eight buckets in two: each chunk is the oracle's for its own earlier download -- with the
    vertices the other chunk has too pinned --, the seams stay open, normals, files and the topology report follow the filled
    chunks, and a finalize brings the chunks back."""
    from mlsgpu_amd import binding as b
    from test_gpu_simplify import CELL, ORIGIN, filled_sink
    mesher, buckets = filled_sink(ctx, 47, lambda k: 0) if chunks == 1 else filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    with pytest.raises(b.InvalidArgument):
        mesher.fill_holes(ALL)                                      # before finalize
    assert buckets == (1 if chunks == 1 else 8) and mesher.finalize() == chunks
    before = [mesher.chunk(i) for i in range(chunks)]
    finalize_stats = mesher.stats()
    shared = rows_of(before[0]["vertices"]) & rows_of(before[1]["vertices"]) if chunks == 2 else set()
    assert chunks == 1 or len(shared) > 100
    masks = [in_rows(c["vertices"], shared) if chunks == 2 else None for c in before]
    mesher.chunk_normals(0)                                         # computed before the call: must not be served after it
    want = [fc.fill(c["vertices"], c["triangles"], ALL, mask) for c, mask in zip(before, masks)]
    st = mesher.fill_holes(ALL)
    assert st == summed([w[2] for w in want]) and mesher.stats() == finalize_stats
    assert st["loops"] == st["filledLoops"] + st["pinnedLoops"] and st["longLoops"] == 0
    if chunks == 2:
        assert st["pinnedLoops"] > 0
    for i in range(chunks):
        c = mesher.chunk(i)
        assert len(c["triangles"]) > 1000 and c["chunk"] == before[i]["chunk"]
        fc.assert_same((c["vertices"], c["triangles"], want[i][2]), want[i])
        assert shared <= boundary_rows(c)                           # the seams are untouched: still boundary in each chunk
        assert tc.report_fields(mesher.chunk_topology(i)) == tc.count_all(len(want[i][0]), want[i][1])
        got = mesher.chunk_normals(i)
        nc.assert_same((got["normals"], got["stats"]), nc.normals(want[i][0], want[i][1]))
        mesher.write_ply(i, tmp_path / "device.ply", comments=("c",))
        b.write_ply(tmp_path / "host.ply", want[i][0], want[i][1], comments=("c",))
        assert file_bytes(tmp_path / "device.ply") == file_bytes(tmp_path / "host.ply")
    with pytest.raises(b.InvalidArgument):
        mesher.fill_holes(2)                                        # a refused parameter costs no results
    assert mesher.chunk(0)["triangles"].tobytes() == want[0][1].tobytes()
    twice = [fc.fill(w[0], w[1], 32, np.concatenate([mask, np.zeros(len(w[0]) - len(mask), bool)]) if chunks == 2 else None)
             for w, mask in zip(want, masks)]
    assert mesher.fill_holes(32) == summed([w[2] for w in twice])   # it may be called again
    for i in range(chunks):
        c = mesher.chunk(i)
        fc.assert_same((c["vertices"], c["triangles"], twice[i][2]), twice[i])
    assert mesher.smooth(2)["numTriangles"] == sum(w[2]["outTriangles"] for w in twice)      # a smooth and a simplify work
    assert mesher.simplify(ORIGIN, CELL)["inTriangles"] == sum(w[2]["outTriangles"] for w in twice)
    assert mesher.finalize() == chunks                              # finalize again: the chunks as they were
    for i in range(chunks):
        c = mesher.chunk(i)
        assert c["vertices"].tobytes() == before[i]["vertices"].tobytes() and c["triangles"].tobytes() == before[i]["triangles"].tobytes()
    mesher.close()


# ---------------------------------------------------------------- reconstruct --fill-holes

def test_reconstruct_fill_holes(ctx, tmp_path):
    """examples/reconstruct --fill-holes 32: one more line, and a file that is the oracle's for the file the same command
    writes without the option -- as a set of positions with the triangles over them, since two runs number their vertices
    in the order their worker threads deliver."""
    from test_gpu_normals import same_mesh
    from test_gpu_simplify import shells
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
    out = subprocess.check_output([exe, "--weld", "device", "--fill-holes", "32"] + args("out.ply"), timeout=300).decode().splitlines()
    assert len(plain) == 1 and len(out) == 2 and out[0] == plain[0], out
    V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
    gotV, gotT = parse_ply_mesh(str(tmp_path / "out.ply"))
    wantV, wantT, st = fc.fill(V, tri, 32)
    assert len(tri) > 100 and same_mesh(gotV, gotT, wantV, wantT)
    line = re.fullmatch(r"fill-holes chunks (\d+) boundary-edges (\d+) loops (\d+) filled (\d+) long (\d+) pinned (\d+) "
                        r"irregular-edges (\d+) vertices (\d+) -> (\d+) triangles (\d+) -> (\d+)", out[1])
    assert line, out[1]
    assert [int(x) for x in line.groups()] == [1, st["boundaryEdges"], st["loops"], st["filledLoops"], st["longLoops"], st["pinnedLoops"],
                                               st["irregularEdges"], len(V), st["outVertices"], len(tri), st["outTriangles"]]
    for bad in ("2", "1048577"):
        refused = subprocess.run([exe, "--weld", "device", "--fill-holes", bad] + args("bad.ply"), capture_output=True, timeout=300)
        assert refused.returncode != 0 and b"--fill-holes takes" in refused.stderr and not (tmp_path / "bad.ply").exists()
    refused = subprocess.run([exe, "--weld", "host", "--fill-holes", "32"] + args("host.ply"), capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--fill-holes needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
