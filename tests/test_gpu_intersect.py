"""mlsgpu_hip_mesh_self_intersections / mlsgpu_hip_mesher_self_intersections on the GPU: every field of the report, every
partner count and the pair list exactly the oracle's (intersect_cases.self_intersections)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import deviation_cases as dc
import fill_cases as fc
import intersect_cases as ic
import sink_cases as sk
import topology_cases as tc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def run(ctx, vertices, triangles, **kw):
    from mlsgpu_amd import binding as b
    return b.mesh_self_intersections(ctx, vertices, np.asarray(triangles).astype(np.uint32), **kw)


def check(ctx, vertices, triangles):
    want = ic.self_intersections(vertices, triangles)
    ic.assert_same(run(ctx, vertices, triangles), want)
    return want


# ---------------------------------------------------------------- hand cases and empty inputs

@pytest.mark.parametrize("case", ic.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(ctx, case):
    name, v, t, crossing = case
    partners, pairs, st = check(ctx, v, t)
    assert st["crossingPairs"] == crossing and st["candidatePairs"] == 1 and pairs.tolist() == ([[0, 1]] if crossing else [])


def test_empty_inputs_and_the_trap(ctx):
    p, tri = fc.grid_mesh(4, 4)
    none = np.zeros((0, 3), np.float32)
    bad = tri.copy()
    bad[3, 1] = 16
    bad[9, 0] = bad[9, 2]
    assert check(ctx, none, tri[:0])[2]["lowestA"] == ic.NONE                    # no vertices, no triangles
    assert check(ctx, none, tri)[2]["outOfRangeTriangles"] == len(tri)          # no vertices
    assert check(ctx, p, tri[:0])[2]["numVertices"] == 16                       # no triangles
    st = check(ctx, p, bad[[3, 9]])[2]                                          # only defective triangles
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["candidatePairs"]) == (1, 1, 0)
    assert check(ctx, p, np.full((5, 3), 7))[2]["degenerateTriangles"] == 5
    assert check(ctx, p, tri[:1])[2]["candidatePairs"] == 0                     # one triangle has no partner
    q, trap = tc.classification_trap()
    st = check(ctx, q, trap)[2]
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["candidatePairs"], st["crossingPairs"]) == (2, 1, 1, 0)
    same = np.tile(np.float32([[3, 4, 5]]), (7, 1))                             # a mesh whose box is one point
    assert check(ctx, same, [[0, 1, 2], [4, 5, 6], [1, 2, 3]])[2]["candidatePairs"] == 3


def jittered():
    return fc.grid_mesh(40, 40, jitter=0.3, seed=3)


def two_sheets():
    p, tri = jittered()
    q, _ = fc.grid_mesh(40, 40, jitter=0.3, seed=4)
    return ic.joined((p, tri), (ic.tilted(q), tri))


def test_two_sheets_and_the_fold(ctx):
    st = check(ctx, *two_sheets())[2]
    assert (st["crossingPairs"], st["crossingTriangles"]) == (223, 213)
    p, tri = jittered()
    assert check(ctx, p, tri)[2]["crossingPairs"] == 0
    p = p.copy()
    p[20 * 40 + 20] += np.float32([3.3, 2.7, 0])
    assert check(ctx, p, tri)[2]["crossingPairs"] == 20
    p[:, 2] = 0
    assert check(ctx, p, tri)[2]["crossingPairs"] == 0                          # the same fold in one plane: nothing is certain


# ---------------------------------------------------------------- many workgroups

HOLES = [(10, 10, 1, 1), (50, 60, 2, 3), (100, 200, 8, 8), (200, 100, 1, 1), (201, 101, 1, 1)]


@pytest.fixture(scope="module")
def big_sheets():
    """The 300 x 300 punched grid with a second, tilted 300 x 300 sheet through it, and the oracle's report."""
    p, tri = fc.punched(300, 300, HOLES, jitter=0.3, seed=11)
    q, qtri = fc.grid_mesh(300, 300, jitter=0.3, seed=12)
    v, t = ic.joined((p, tri), (ic.tilted(q, 0.5, 150.3), qtri))
    assert len(t) > 356_000
    want = ic.self_intersections(v, t)
    assert want[2]["crossingPairs"] > 1000 and want[2]["maxPartners"] >= 3
    return v, t, want


def test_many_workgroups(ctx, big_sheets):
    v, t, want = big_sheets
    for _ in range(3):
        ic.assert_same(run(ctx, v, t), want)
    partners, pairs, st = run(ctx, v, t, want_partners=False, want_pairs=False)
    assert partners is None and pairs is None
    ic.same_stats(st, want[2])


def test_shuffled_triangles(ctx, big_sheets):
    """The order of the triangles changes only which indices are named."""
    v, t, want = big_sheets
    order = np.random.default_rng(3).permutation(len(t))                        # shuffled[k] = t[order[k]]
    partners, pairs, st = run(ctx, v, t[order])
    for name in ("candidatePairs", "crossingPairs", "crossingTriangles", "maxPartners", "outOfRangeTriangles", "degenerateTriangles"):
        assert st[name] == want[2][name], name
    np.testing.assert_array_equal(partners, want[0][order])
    back = np.sort(order[pairs.astype(np.int64)], axis=1)
    back = back[np.lexsort((back[:, 1], back[:, 0]))]
    np.testing.assert_array_equal(back, want[1])
    assert (np.diff(pairs[:, 0].astype(np.int64) << 32 | pairs[:, 1]) > 0).all() and (pairs[:, 0] < pairs[:, 1]).all()
    assert [st["lowestA"], st["lowestB"]] == pairs[0].tolist()
    assert st["maxPartnersTriangle"] == int(np.argmax(partners))


# ---------------------------------------------------------------- the shapes of the grid

def test_one_cell_holds_everything(ctx):
    """A 40 x 40 grid and a tilted copy of it scaled down to a third of a unit: the mean extent of a box, which sizes the
    cell, is more than the whole copy, so one cell holds its 3 042 triangles and the grid's triangles there."""
    p, tri = jittered()
    small = ((ic.tilted(p).astype(np.float64) - [19.37, 19.37, 0.0]) / 128.0 + [20.4, 20.4, 0.0]).astype(np.float32)
    v, t = ic.joined((p, tri), (small, tri))
    st = check(ctx, v, t)[2]
    assert st["crossingPairs"] > 50 and st["maxPartners"] > 20


def test_a_cell_with_thousands_of_triangles(ctx):
    """A fan of 5 000 triangles around one vertex, every one in the centre's cell, and 50 long needles through the centre."""
    v, t = ic.joined(dc.fan(5000, seed=1), ic.needles(50, seed=2))
    st = check(ctx, v, t)[2]
    assert st["candidatePairs"] > 5000 * 4999 // 2 and st["crossingPairs"] > 5000 and st["maxPartners"] > 100


def test_one_triangle_spans_the_grid(ctx):
    """19 800 small triangles and one giant, tilted one through them whose box holds the whole grid and more: at the first
    cell size it alone would go into millions of cells, so the cell is doubled -- the count kernel runs more than once."""
    p, tri = fc.grid_mesh(100, 101, jitter=0.2, seed=5)
    assert len(tri) == 19_800
    giant = np.float32([[-50, -50, -50], [160, 0, 150], [0, 160, 100]])
    t = np.concatenate([tri, [[len(p), len(p) + 1, len(p) + 2]]])
    # that test's triangle: its box holds the grid, its plane leaves z = 0 just outside the grid's corner -- every small
    # triangle is its candidate and none crosses it; and the same triangle moved so that it cuts through the grid
    for shift, crossing in (((0, 0, 0), False), ((60, 60, 0), True)):
        v = np.concatenate([p, giant + np.float32(shift)])
        ctx.reset_stats()
        ctx.set_timing(True)
        try:
            want = check(ctx, v, t)
        finally:
            ctx.set_timing(False)
        stats = ctx.stats()
        assert stats["kernel.intersect.count"][1] >= 2
        assert stats["intersect.scratch.bytes"][0] > 24 * stats["intersect.records"][0]
        assert want[2]["candidatePairs"] > 100_000 + len(tri)
        if crossing:
            assert want[2]["maxPartnersTriangle"] == len(tri) and want[2]["maxPartners"] > 100
            assert want[2]["crossingPairs"] == want[2]["maxPartners"] and (want[1][:, 1] == len(tri)).all()
        else:
            assert want[2]["crossingPairs"] == 0


def test_beyond_the_one_launch_scan(ctx):
    """The scan over the triangles' cell counts takes its two-launch form beyond 1 024 tiles of 2 048: 2.1 M triangles, and a
    30 x 30 sheet through them."""
    p, tri = fc.grid_mesh(1030, 1030, jitter=0.2, seed=8)
    assert len(tri) > 1024 * 2048
    q, qtri = fc.grid_mesh(30, 30, jitter=0.2, seed=9)
    sheet = ic.tilted(q, 0.5, 14.6) + np.float32([500, 500, 0])
    st = check(ctx, *ic.joined((p, tri), (sheet, qtri)))[2]
    assert 50 < st["crossingPairs"] < 2000


# ---------------------------------------------------------------- capacity, untouched memory

def test_capacity_guard_bands_and_inputs(ctx):
    from mlsgpu_amd import binding as b
    v, t = two_sheets()
    want = ic.self_intersections(v, t)
    N, T, G = want[2]["crossingPairs"], len(t), 512
    assert N == 223
    dv, dt = b.DeviceBuffer(ctx, array=v), b.DeviceBuffer(ctx, array=t.astype(np.uint32))
    band_p, band_l = np.full(2 * G + T, 0xDEADBEEF, np.uint32), np.full(2 * G + 2 * (N + 7), 0xFEEDF00D, np.uint32)
    op, ol = b.DeviceBuffer(ctx, array=band_p), b.DeviceBuffer(ctx, array=band_l)

    def call(with_partners, with_pairs, capacity):
        st = b.SelfIntersections()
        rc = b.lib().mlsgpu_hip_mesh_self_intersections(ctx.h, dv.ptr, len(v), dt.ptr, T, op.ptr + 4 * G if with_partners else None,
                                                        ol.ptr + 4 * G if with_pairs else None, capacity, C.byref(st))
        return rc, st.as_dict()

    rc, st = call(False, False, 0)                                  # the report alone is the same report
    assert rc == 0
    ic.same_stats(st, want[2])
    assert op.download(np.uint32).tobytes() == band_p.tobytes() and ol.download(np.uint32).tobytes() == band_l.tobytes()
    rc, st = call(False, False, 10 ** 6)                            # a capacity without a list asks for nothing
    assert rc == 0
    for capacity in (0, N - 1):                                     # too small: the complete report, the list untouched
        rc, st = call(True, True, capacity)
        with pytest.raises(b.LengthError):
            b.check(rc)
        ic.same_stats(st, want[2])
        assert ol.download(np.uint32).tobytes() == band_l.tobytes()
        got = op.download(np.uint32)
        assert got[:G].tobytes() == band_p[:G].tobytes() and got[G + T:].tobytes() == band_p[G + T:].tobytes()
        np.testing.assert_array_equal(got[G:G + T], want[0])
    for capacity in (N, N + 7):                                     # enough, and more than enough: N rows and no more
        ol.upload(band_l)
        op.upload(band_p)
        rc, st = call(True, True, capacity)
        assert rc == 0
        got_p, got_l = op.download(np.uint32), ol.download(np.uint32)
        assert got_p[:G].tobytes() == band_p[:G].tobytes() and got_p[G + T:].tobytes() == band_p[G + T:].tobytes()
        assert got_l[:G].tobytes() == band_l[:G].tobytes() and got_l[G + 2 * N:].tobytes() == band_l[G + 2 * N:].tobytes()
        ic.assert_same((got_p[G:G + T], got_l[G:G + 2 * N], st), want)
    assert dv.download(np.float32).tobytes() == v.tobytes() and dt.download(np.uint32).tobytes() == t.astype(np.uint32).tobytes()
    for buf in (dv, dt, op, ol):
        buf.free()


# ---------------------------------------------------------------- defects and errors

def test_defects(ctx):
    v, t = two_sheets()
    bad = dc.sprinkled(t, len(v))
    st = check(ctx, v, bad)[2]
    assert st["outOfRangeTriangles"] > 200 and st["degenerateTriangles"] > 100 and 0 < st["crossingPairs"] < 223


def small_correct_call(ctx):
    name, v, t, crossing = ic.hand_cases()[0]
    assert check(ctx, v, t)[2]["crossingPairs"] == crossing


def test_errors_leave_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    p, tri = fc.grid_mesh(9, 11, jitter=0.2, seed=3)
    q = p.copy()
    q[7, 2] = np.nan
    q[50, 0] = -np.inf
    with pytest.raises(ic.Invalid):
        ic.self_intersections(q, tri)
    with pytest.raises(b.InvalidArgument, match="2 vertex coordinates are not finite"):
        run(ctx, q, tri)
    small_correct_call(ctx)
    q[98, 1] = np.inf                                               # a vertex no triangle uses is refused all the same
    with pytest.raises(b.InvalidArgument, match="3 vertex coordinates are not finite"):
        run(ctx, q, tri[:4])
    small_correct_call(ctx)
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st = b.SelfIntersections()
    for n_vertices, n_triangles in ((2 ** 32, 1), (1, (2 ** 32 + 2) // 3)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_self_intersections(ctx.h, one.ptr, n_vertices, one.ptr, n_triangles, None, None, 0,
                                                               C.byref(st)))
        small_correct_call(ctx)
    one.free()


# ---------------------------------------------------------------- the device sink

def test_sink(ctx, tmp_path):
    """A sheet in two chunks: the report is the oracle's per-chunk reports combined, and the call changes nothing."""
    from mlsgpu_amd import binding as b
    from test_gpu_deviation import filled, state_of
    meshes = sk.tiled_sheet(21, 48, 48, 8, 0.15, 0.3, 2)
    sink = filled(ctx, meshes)
    with pytest.raises(b.InvalidArgument):
        sink.self_intersections()                                   # before finalize
    assert sink.finalize() == 2

    def against_the_oracle():
        now = [sink.chunk(i) for i in range(2)]
        assert all(len(c["triangles"]) > 100 for c in now)
        before = state_of(sink, 2, tmp_path)
        got = b.mesher_self_intersections(sink)
        assert state_of(sink, 2, tmp_path) == before
        ic.same_stats(got, ic.combined([ic.self_intersections(c["vertices"], c["triangles"])[2] for c in now]))
        assert got == sink.self_intersections()
        return got

    st = against_the_oracle()
    assert st["candidatePairs"] > st["numTriangles"] and st["crossingPairs"] == 0 and st["lowestA"] == ic.NONE
    sink.simplify((-1.0, -1.0, -1.0), 3.0)
    assert against_the_oracle()["numTriangles"] < st["numTriangles"]
    sink.smooth(3)
    against_the_oracle()
    sink.close()


# ---------------------------------------------------------------- reconstruct --self-intersections

def test_reconstruct_self_intersections(ctx, tmp_path):
    """examples/reconstruct --self-intersections: one more line, and the same file."""
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

    with_flag = subprocess.check_output([exe, "--weld", "device", "--simplify", "4", "--self-intersections"] + args("out.ply"), timeout=300)
    with_flag = with_flag.decode().splitlines()
    plain = subprocess.check_output([exe, "--weld", "device", "--simplify", "4"] + args("plain.ply"), timeout=300).decode().splitlines()
    assert len(with_flag) == 3 and with_flag[:2] == plain, with_flag
    m = re.fullmatch(r"self-intersections pairs (\d+) triangles (\d+) chunks (\d+) first (-|\d+ \d+ \d+)", with_flag[2])
    assert m, with_flag[2]
    pairs, triangles, chunks = (int(x) for x in m.groups()[:3])
    if pairs:
        c, a, b_ = (int(x) for x in m.group(4).split())
        assert a < b_ and c >= 0 and 2 <= triangles <= 2 * pairs and chunks >= 1
    else:
        assert m.group(4) == "-" and triangles == 0 and chunks == 0
    assert (tmp_path / "out.ply").read_bytes() == (tmp_path / "plain.ply").read_bytes()
    refused = subprocess.run([exe, "--weld", "host", "--self-intersections"] + args("host.ply"), capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--self-intersections needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
