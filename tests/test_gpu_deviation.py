"""mlsgpu_hip_mesh_deviation / mlsgpu_hip_mesher_deviation on the GPU: every distance, every nearest triangle and every field of
the report bit for bit the oracle's (deviation_cases.deviation)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import deviation_cases as dc
import fill_cases as fc
import simplify_cases as sc
import sink_cases as sk
import topology_cases as tc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def run(ctx, points, vertices, triangles, D, **kw):
    from mlsgpu_amd import binding as b
    return b.mesh_deviation(ctx, points, vertices, np.asarray(triangles).astype(np.uint32), D, **kw)


def check(ctx, points, vertices, triangles, D):
    want = dc.deviation(points, vertices, triangles, D)
    dc.assert_same(run(ctx, points, vertices, triangles, D), want)
    return want


# ---------------------------------------------------------------- hand cases and empty inputs

@pytest.mark.parametrize("case", dc.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(ctx, case):
    name, p, v, t, D = case
    d, near, st = check(ctx, p, v, t, D)
    if name in dc.HAND_ANSWERS:
        assert d.tolist() == [dc.HAND_ANSWERS[name]] and near.tolist() == [0]
    else:
        assert near.tolist() == [0, dc.NO_TRIANGLE]


def test_the_limit_and_the_trap(ctx):
    p, v, t = np.array([[1, 1, 2]], np.float32), dc.RIGHT, [[0, 1, 2]]
    assert check(ctx, p, v, t, 2.0)[2]["histogram"] == [0] * 15 + [1]         # best == D2: within, in the last bin
    assert check(ctx, p, v, t, np.nextafter(np.float32(2.0), np.float32(0.0)))[2]["beyond"] == 1
    heights = np.stack([np.ones(17), np.ones(17), np.arange(17)], axis=1).astype(np.float32)
    assert check(ctx, heights, v, t, 16.0)[2]["histogram"] == [1] * 15 + [2]
    q, tri = tc.classification_trap()
    st = check(ctx, q, q, tri, 1.0)[2]
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["within"]) == (2, 1, 4)


def test_empty_inputs(ctx):
    p, tri = fc.grid_mesh(4, 4)
    none = np.zeros((0, 3), np.float32)
    bad = tri.copy()
    bad[3, 1] = 16
    bad[9, 0] = bad[9, 2]
    st = check(ctx, none, p, bad, 2.0)[2]                                       # no points: the triangle counts are still made
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["scaleExponent"], st["farthestPoint"]) == (1, 1, 0, dc.NO_POINT)
    assert check(ctx, none, none, tri[:0], 2.0)[2]["limit2"] == 4.0
    for target in ((none, tri), (p, tri[:0]), (p, np.full((5, 3), 7)), (p, bad[[3, 9]])):
        st = check(ctx, p, *target, 2.0)[2]                                     # no triangle takes part: every point beyond
        assert (st["within"], st["beyond"], st["scaleExponent"]) == (0, 16, 2)
    same = np.tile(np.float32([[3, 4, 5]]), (7, 1))                             # a target whose box is one point
    assert check(ctx, same + np.float32(1), same, [[0, 1, 2], [4, 5, 6]], 2.0)[2]["within"] == 7


# ---------------------------------------------------------------- many workgroups

HOLES = [(10, 10, 1, 1), (50, 60, 2, 3), (100, 200, 8, 8), (200, 100, 1, 1), (201, 101, 1, 1)]
DISTANCES = (0.05, 0.5, 6.0)


@pytest.fixture(scope="module")
def big_grid():
    """The 300 x 300 jittered grid, its clustering at cell 3, and the oracle's reports in both directions."""
    p, tri = fc.punched(300, 300, HOLES, jitter=0.3, seed=11)
    sv, stri, _ = sc.simplify(p, tri, (-1.0, -1.0, -1.0), 3.0)
    assert p.shape == (90_000, 3) and len(tri) > 178_000 and len(sv) % 64 != 0 and len(sv) > 10_000
    want = {}
    for D in DISTANCES:
        want[D, "moved"] = dc.deviation(sv, p, tri, D)
        want[D, "lost"] = dc.deviation(p, sv, stri, D)
    return dict(moved=(sv, p, tri), lost=(p, sv, stri)), want


@pytest.mark.parametrize("direction", ["moved", "lost"])
@pytest.mark.parametrize("D", DISTANCES)
def test_clustered_grid(ctx, big_grid, D, direction):
    """Some 40 workgroups of points against 178 k small triangles, and 350 against 22 k triangles that span many cells at a
    small D.  At 0.05 most points are beyond, at 0.5 a few, at 6 none."""
    meshes, want = big_grid
    st = want[D, direction][2]
    if D == 0.05:
        assert st["beyond"] > 0 and st["within"] > 0
    elif D == 0.5:
        assert st["within"] > 0 and st["beyond"] > 0
    else:
        assert st["beyond"] == 0 and st["maxDistance2"] > 1.0
    dc.assert_same(run(ctx, *meshes[direction], D), want[D, direction])


def test_determinism_and_optional_outputs(ctx, big_grid):
    meshes, want = big_grid
    runs = [run(ctx, *meshes["lost"], 0.5) for _ in range(3)]
    for r in runs:
        dc.assert_same(r, want[0.5, "lost"])
    d, near, st = run(ctx, *meshes["lost"], 0.5, want_distances=False, want_nearest=False)
    assert d is None and near is None
    dc.same_stats(st, want[0.5, "lost"][2])
    order = np.random.default_rng(3).permutation(len(meshes["lost"][2]))      # the order of the triangles names other triangles only
    d, near, st = run(ctx, meshes["lost"][0], meshes["lost"][1], meshes["lost"][2][order], 0.5)
    dc.assert_same((d, None, st), want[0.5, "lost"])


@pytest.mark.parametrize("lanes", [1, 2, 16, 64])
def test_lanes_per_point(ctx, big_grid, monkeypatch, lanes):
    """The distance kernel deals a point's pairs out to 1 .. 64 lanes by the number of points (10 156 points take 64, 90 000
    take 8, 600 000 would take one); here every width is forced on both directions, ties between lanes included."""
    meshes, want = big_grid
    monkeypatch.setenv("MLSGPU_HIP_DEVIATION_LANES", str(lanes))
    dc.assert_same(run(ctx, *meshes["lost"], 0.5), want[0.5, "lost"])
    dc.assert_same(run(ctx, *meshes["moved"], 6.0), want[6.0, "moved"])
    sv, p, tri = meshes["moved"]
    d, near, st = run(ctx, sv, p, np.concatenate([tri, tri[::-1]]), 0.5)       # every distance twice, often in two lanes:
    dc.assert_same((d, near, dict(st, numTriangles=len(tri))), want[0.5, "moved"])      # the copy in the first half is named


# ---------------------------------------------------------------- the shapes of the grid

def test_one_cell_holds_everything(ctx):
    """D = 1000 over a 40 x 40 grid: one cell, every pair a candidate, 4.9 M of them."""
    p, tri = fc.grid_mesh(40, 40, jitter=0.3, seed=3)
    q = (p + np.random.default_rng(4).uniform(-2, 2, p.shape)).astype(np.float32)
    st = check(ctx, q, p, tri, 1000.0)[2]
    assert st["within"] == 1600 and st["histogram"][0] == 1600


def test_a_cell_with_thousands_of_triangles(ctx):
    """A fan of 5 000 triangles around one vertex: every triangle lies in the centre's cell, and 3 000 points walk them."""
    v, tri = dc.fan(5000, seed=1)
    p = np.random.default_rng(2).uniform(0, 1, (3000, 3)).astype(np.float32)
    st = check(ctx, p, v, tri, 0.01)[2]
    assert st["within"] > 1000 and st["beyond"] > 100


def test_one_triangle_spans_the_grid(ctx):
    """20 000 small triangles under one giant, tilted one whose box holds the whole grid and more: at the first cell size
    (the mean extent of a triangle's box, about 1.2) it alone would go into some 4 * 10^6 cells, beyond the budget of 2^20
    pairs, so the cell is doubled -- the count kernel runs more than once."""
    p, tri = fc.grid_mesh(100, 101, jitter=0.2, seed=5)
    assert len(tri) == 19_800
    v = np.concatenate([p, [[-50, -50, -50], [160, 0, 150], [0, 160, 100]]]).astype(np.float32)
    t = np.concatenate([tri, [[len(p), len(p) + 1, len(p) + 2]]])
    q = np.concatenate([p + np.float32(0.1), np.random.default_rng(6).uniform(-5, 110, (5000, 3)).astype(np.float32)])
    ctx.reset_stats()
    ctx.set_timing(True)
    try:
        want = check(ctx, q, v, t, 0.25)
    finally:
        ctx.set_timing(False)
    assert ctx.stats()["kernel.deviation.count"][1] >= 2
    assert want[2]["within"] > 10_000 and want[2]["beyond"] > 1000 and (want[1] == len(tri)).sum() > 3


def test_beyond_the_one_launch_scan(ctx):
    """The scan over the triangles' cell counts takes its two-launch form beyond 1 024 tiles of 2 048: 2.1 M triangles."""
    p, tri = fc.grid_mesh(1030, 1030, jitter=0.2, seed=8)
    assert len(tri) > 1024 * 2048
    rng = np.random.default_rng(9)
    q = (p[rng.choice(len(p), 3000, replace=False)] + rng.uniform(-0.4, 0.4, (3000, 3))).astype(np.float32)
    st = check(ctx, q, p, tri, 0.3)[2]
    assert st["within"] > 1000 and st["beyond"] > 100


def test_points_outside_the_grid(ctx):
    """Points far from the target's box are clamped into border cells and fail step 2 there; with a D that reaches them they
    are found."""
    p, tri = fc.grid_mesh(12, 9, jitter=0.2, seed=2)
    q = np.array([[100, 100, 100], [-50, 2, 0], [5, 4, -1e6], [5, 4, 0.5], [3e38, 0, 0]], np.float32)
    assert check(ctx, q, p, tri, 1.0)[2]["beyond"] == 4
    assert check(ctx, q[:2], p, tri, 200.0)[2]["within"] == 2


def test_the_mesh_twice(ctx, big_grid):
    meshes, want = big_grid
    sv, p, tri = meshes["moved"]
    d, near, st = run(ctx, sv, p, np.concatenate([tri, tri]), 0.5)
    assert (near[near != dc.NO_TRIANGLE] < len(tri)).all() and st["numTriangles"] == 2 * len(tri)
    dc.assert_same((d, near, dict(st, numTriangles=len(tri))), want[0.5, "moved"])


# ---------------------------------------------------------------- defects and errors

def test_defects(ctx):
    p, tri = fc.punched(30, 41, [(5, 5, 1, 1), (12, 20, 2, 2)], jitter=0.2, seed=9)
    bad = dc.sprinkled(tri, len(p))
    q = (p + np.random.default_rng(1).uniform(-0.4, 0.4, p.shape)).astype(np.float32)
    st = check(ctx, q, p, bad, 0.3)[2]
    assert st["outOfRangeTriangles"] == 220 and st["degenerateTriangles"] == 110 and st["within"] > 0 and st["beyond"] > 0


def small_correct_call(ctx):
    check(ctx, *dc.hand_cases()[0][1:])


def test_errors_leave_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    p, tri = fc.grid_mesh(9, 11, jitter=0.2, seed=3)
    for D in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(dc.Invalid):
            dc.deviation(p, p, tri, D)
        with pytest.raises(b.InvalidArgument):
            run(ctx, p, p, tri, D)
        small_correct_call(ctx)
    q = p.copy()
    q[7, 2] = np.nan
    q[50, 0] = -np.inf
    with pytest.raises(b.InvalidArgument, match="2 point and 0 target coordinates are not finite"):
        run(ctx, q, p, tri, 1.0)
    small_correct_call(ctx)
    with pytest.raises(b.InvalidArgument, match="0 point and 2 target coordinates are not finite"):
        run(ctx, p, q, tri, 1.0)
    small_correct_call(ctx)
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st = b.Deviation()
    for n_points, n_vertices, n_triangles in ((2 ** 32, 1, 1), (1, 2 ** 32, 1), (1, 1, (2 ** 32 + 2) // 3)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_deviation(ctx.h, one.ptr, n_points, one.ptr, n_vertices, one.ptr, n_triangles, 1.0, None, None,
                                                      C.byref(st)))
    one.free()
    small_correct_call(ctx)


# ---------------------------------------------------------------- untouched memory

def test_guard_bands_and_inputs(ctx):
    from mlsgpu_amd import binding as b
    p, tri = fc.punched(61, 67, [(3, 3, 1, 1), (20, 30, 3, 4)], jitter=0.25, seed=4)
    q = (p[::3] + np.random.default_rng(7).uniform(-0.5, 0.5, p[::3].shape)).astype(np.float32)
    want = dc.deviation(q, p, tri, 0.4)
    P, G = len(q), 512
    assert want[2]["within"] > 100 and want[2]["beyond"] > 100
    dq, dv, dt = b.DeviceBuffer(ctx, array=q), b.DeviceBuffer(ctx, array=p), b.DeviceBuffer(ctx, array=tri.astype(np.uint32))
    band_d, band_n = np.full(2 * G + P, -123.25, np.float64), np.full(2 * G + P, 0xDEADBEEF, np.uint32)
    od, on = b.DeviceBuffer(ctx, array=band_d), b.DeviceBuffer(ctx, array=band_n)

    def call(with_distances, with_nearest):
        st = b.Deviation()
        b.check(b.lib().mlsgpu_hip_mesh_deviation(ctx.h, dq.ptr, P, dv.ptr, len(p), dt.ptr, len(tri), 0.4,
                                                  od.ptr + 8 * G if with_distances else None, on.ptr + 4 * G if with_nearest else None,
                                                  C.byref(st)))
        return st.as_dict()

    dc.same_stats(call(False, False), want[2])                      # the report alone is the same report
    assert od.download(np.float64).tobytes() == band_d.tobytes() and on.download(np.uint32).tobytes() == band_n.tobytes()
    dc.same_stats(call(True, False), want[2])
    assert on.download(np.uint32).tobytes() == band_n.tobytes()
    st = call(True, True)
    got_d, got_n = od.download(np.float64), on.download(np.uint32)
    for got, band in ((got_d, band_d), (got_n, band_n)):
        assert got[:G].tobytes() == band[:G].tobytes() and got[G + P:].tobytes() == band[G + P:].tobytes()
    dc.assert_same((got_d[G:G + P], got_n[G:G + P], st), want)
    assert dq.download(np.float32).tobytes() == q.tobytes() and dv.download(np.float32).tobytes() == p.tobytes()
    assert dt.download(np.uint32).tobytes() == tri.astype(np.uint32).tobytes()
    for buf in (dq, dv, dt, od, on):
        buf.free()


# ---------------------------------------------------------------- the device sink

def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def filled(ctx, meshes):
    import mlsgpu_amd as m
    sink = m.Mesher(ctx, 0.0)
    seen = {}
    for mesh in meshes:
        sink.add(seen.setdefault(mesh["chunk"], len(seen)), mesh["vertices"], mesh["num_internal"], mesh["keys"], mesh["triangles"])
    return sink


def state_of(sink, chunks, tmp_path):
    """Everything a caller can see of the sink's chunks: arrays, topology reports, files."""
    out = []
    for i in range(chunks):
        c = sink.chunk(i)
        sink.write_ply(i, tmp_path / "state.ply", comments=("c",))
        out.append((c["chunk"], c["vertices"].tobytes(), c["triangles"].tobytes(), tc.report_fields(sink.chunk_topology(i)),
                    file_bytes(tmp_path / "state.ply")))
    return out


def test_sink(ctx, tmp_path):
    """A sheet in two chunks: the reports are the oracle's per-chunk reports added up, and the calls change nothing."""
    from mlsgpu_amd import binding as b
    meshes = sk.tiled_sheet(21, 48, 48, 8, 0.15, 0.3, 2)
    D, origin, cell = 6.0, (-1.0, -1.0, -1.0), 3.0
    sink = filled(ctx, meshes)
    with pytest.raises(b.InvalidArgument):
        sink.keep_reference()                                       # before finalize
    assert sink.finalize() == 2
    with pytest.raises(b.InvalidArgument):
        sink.deviation(D)                                           # nothing kept
    kept = [sink.chunk(i) for i in range(2)]
    before = state_of(sink, 2, tmp_path)
    sink.keep_reference()
    moved, lost = sink.deviation(D)
    assert state_of(sink, 2, tmp_path) == before
    for st in (moved, lost):
        assert st["within"] == st["numPoints"] == sum(len(c["vertices"]) for c in kept) and st["beyond"] == 0
        assert st["maxDistance2"] == 0.0 and st["sumQ"] == 0 and st["histogram"][0] == st["within"]
        assert (st["farthestChunk"], st["farthestPoint"]) == (0, 0)
    for D_bad in (0.0, np.nan):
        with pytest.raises(b.InvalidArgument):
            sink.deviation(D_bad)

    def against_the_oracle():
        now = [sink.chunk(i) for i in range(2)]
        assert all(len(c["triangles"]) > 100 for c in now)
        before = state_of(sink, 2, tmp_path)
        moved, lost = b.mesher_deviation(sink, D)
        assert state_of(sink, 2, tmp_path) == before
        want_moved = dc.combined([dc.deviation(n["vertices"], k["vertices"], k["triangles"], D)[2] for n, k in zip(now, kept)])
        want_lost = dc.combined([dc.deviation(k["vertices"], n["vertices"], n["triangles"], D)[2] for n, k in zip(now, kept)])
        dc.same_stats(moved, want_moved)
        dc.same_stats(lost, want_lost)
        return moved, lost

    sink.simplify(origin, cell)
    moved, lost = against_the_oracle()
    assert moved["maxDistance2"] > 0 and lost["maxDistance2"] > 0 and moved["numPoints"] < lost["numPoints"]
    sink.smooth(3)
    against_the_oracle()
    assert sink.finalize() == 2                                     # the same chunk list: the reference stays
    moved, _ = sink.deviation(D)
    assert moved["maxDistance2"] == 0.0 and moved["within"] == lost["numPoints"]
    sink.drop_reference()
    with pytest.raises(b.InvalidArgument):
        sink.deviation(D)
    sink.keep_reference()
    sink.reset()                                                    # the reference goes with the job
    for mesh in meshes[:40]:
        sink.add(0, mesh["vertices"], mesh["num_internal"], mesh["keys"], mesh["triangles"])
    assert sink.finalize() == 1
    with pytest.raises(b.InvalidArgument):
        sink.deviation(D)
    sink.close()


# ---------------------------------------------------------------- reconstruct --deviation

def test_reconstruct_deviation(ctx, tmp_path):
    """examples/reconstruct --simplify 4 --deviation D: two more lines whose counts add up to the vertex counts."""
    from test_gpu_simplify import shells
    from test_host_cpp import build_example
    from mlsgpu_amd import synth
    exe = build_example(tmp_path, "reconstruct")
    cloud = shells()
    rows = np.zeros(len(cloud), synth.PLY_ROW)
    rows["p"], rows["n"], rows["r"] = cloud["position"], cloud["normal"], cloud["radius"]
    (tmp_path / "in.ply").write_bytes(synth.ply_header(len(rows)) + rows.tobytes())

    def args(out):
        return [str(tmp_path / "in.ply"), str(tmp_path / out), "1.0", "1.5", "4", "3", "0.02", "8000"]

    out = subprocess.check_output([exe, "--weld", "device", "--simplify", "4", "--deviation", "7"] + args("out.ply"), timeout=300)
    out = out.decode().splitlines()
    assert len(out) == 4, out
    sizes = re.fullmatch(r"simplify cell \S+ origin \S+ \S+ \S+ vertices (\d+) -> (\d+) triangles .*", out[1])
    assert sizes, out[1]
    before, after = (int(x) for x in sizes.groups())
    pattern = r"deviation %s points (\d+) within (\d+) beyond (\d+) max (\S+) rms (\S+) p50 (\S+) p90 (\S+)"
    for line, name, points in ((out[2], "moved", after), (out[3], "lost", before)):
        m = re.fullmatch(pattern % name, line)
        assert m, line
        n, within, beyond = (int(x) for x in m.groups()[:3])
        top, rms, p50, p90 = (float(x) for x in m.groups()[3:])
        assert n == points == within + beyond and within > 0 and 0 < rms <= top <= 7.0 and 0 < p50 <= p90 <= 7.0
    plain = subprocess.check_output([exe, "--weld", "device", "--deviation", "1"] + args("plain.ply"), timeout=300).decode().splitlines()
    assert len(plain) == 3 and re.fullmatch(pattern % "moved", plain[1]).groups()[2:5] == ("0", "0", "0")     # no lossy stage
    refused = subprocess.run([exe, "--weld", "host", "--deviation", "1"] + args("host.ply"), capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--deviation needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
    refused = subprocess.run([exe, "--weld", "device", "--deviation", "0"] + args("bad.ply"), capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--deviation takes" in refused.stderr and not (tmp_path / "bad.ply").exists()
