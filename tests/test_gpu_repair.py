"""mlsgpu_hip_mesh_repair / mlsgpu_hip_mesher_repair on the GPU: every result bit for bit the oracle's (repair_cases.repair)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import fill_cases as fc
import normals_cases as nc
import repair_cases as rc
import simplify_cases as sc
import topology_cases as tc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

FLAGS = (0, rc.SPLIT_PINCHES)


def run(ctx, vertices, triangles, flags=0):
    from mlsgpu_amd import binding as b
    return b.mesh_repair(ctx, vertices, np.asarray(triangles).astype(np.uint32).reshape(-1, 3), flags, with_source=True)


def check(ctx, vertices, triangles, flags=0, want=None):
    want = rc.repair(vertices, triangles, flags) if want is None else want
    rc.assert_same(run(ctx, vertices, triangles, flags), want)
    return want


def manifold(ctx, vertices, triangles):
    from mlsgpu_amd import binding as b
    return tc.report_fields(b.mesh_topology(ctx, np.asarray(triangles, np.uint32), len(vertices)))


# ---------------------------------------------------------------- hand cases and empty meshes

def test_hand_cases_and_empty_meshes(ctx):
    p, tri = rc.bowtie(4, 5)
    for flags in FLAGS:
        v, t, st, src = run(ctx, p, tri, flags)
        assert src.tolist() == [0, 0] + list(range(1, 10)) and v.tobytes() == p[src].tobytes()
        assert t.tolist() == [[0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 2], [1, 6, 7], [1, 7, 8], [1, 8, 9], [1, 9, 10], [1, 10, 6]]
        assert (st["splitVertices"], st["addedVertices"], st["outVertices"], st["outTriangles"]) == (1, 1, 11, 9)
    p, tri = rc.two_fans(2, 3)
    assert run(ctx, p, tri, 0)[1].tolist() == tri.tolist()          # two boundary runs at one vertex: left alone
    assert run(ctx, p, tri, rc.SPLIT_PINCHES)[1].tolist() == [[0, 2, 3], [0, 3, 4], [1, 5, 6], [1, 6, 7], [1, 7, 8]]
    extra = np.concatenate([rc.fan(2, 0, 1), tc.cone(4, 0, 4), rc.fan(2, 0, 8)])
    meshes = [rc.bowtie(4, 5), rc.bowtie(4, 5, hub=6), rc.cone_and_fan(), rc.two_fans(), rc.fin(), rc.twice(), (rc.positions(11, 4), extra),
              tc.classification_trap(), rc.torus_mesh(7, 5, 0.5, 0.125)]
    for p, tri in meshes:
        for flags in FLAGS:
            want = check(ctx, p, tri, flags)
            assert manifold(ctx, want[0], want[1])["count"] == [0] * 6
    p, tri = rc.grid_mesh(4, 4)
    for flags in FLAGS:
        assert not any(check(ctx, p[:0], tri[:0], flags)[2].values())                   # V = 0 and T = 0
        assert check(ctx, p[:0], tri, flags)[2]["outOfRangeTriangles"] == 18            # V = 0: every index is out of range
        assert check(ctx, p, tri[:0], flags)[2]["unusedVertices"] == 16                 # T = 0: every vertex goes
        bad = np.array([[0, 1, 99], [5, 5, 6], [16, 0, 1], [3, 3, 3]])
        st = check(ctx, p, bad, flags)[2]                                               # all triangles bad
        assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["outVertices"], st["outTriangles"]) == (2, 2, 0, 0)
        st = check(ctx, p, np.concatenate([tri, tri]), flags)[2]                        # every triangle dropped
        assert (st["repeatedSides"], st["droppedTriangles"], st["unusedVertices"], st["outVertices"]) == (108, 36, 16, 0)
    q = p.copy()
    q[5] = [np.nan, np.inf, -0.0]                                                       # positions are copied, not looked at
    v, _, _, _ = check(ctx, q, tri, 0)
    assert v.tobytes() == q.tobytes()


def test_random_meshes(ctx):
    """A few hundred of the oracle test's draws, laid side by side as one mesh so that one call checks them all."""
    rng = np.random.default_rng(5)
    ps, ts, base = [], [], 0
    for _ in range(400):
        V, tri = tc.random_mesh(rng)
        tri = np.where(tri >= V, 10 ** 6, tri + base)               # out of range stays out of range
        ps.append(rc.positions(V, 7) + np.float32(base))
        ts.append(tri)
        base += V
    p, tri = np.concatenate(ps), np.concatenate(ts)
    for flags in FLAGS:
        want = check(ctx, p, tri, flags)
        assert want[2]["splitVertices"] > 20 and want[2]["droppedTriangles"] > 100 and want[2]["outOfRangeTriangles"] > 10
        assert manifold(ctx, want[0], want[1])["manifold"] == 1


# ---------------------------------------------------------------- many tiles

@pytest.fixture(scope="module")
def big_torus():
    """A torus of 300 000 vertices clustered to 170 484: 3 T = 1 023 240 records are 250 sort tiles of 4 096 and 500 scan tiles,
    the last of each partial, and neither 3 T nor V is a multiple of 64."""
    p, tri = rc.simplified_torus(1500, 200, 0.05, 0.0025)
    assert 3 * len(tri) > 100 * 4096 and 3 * len(tri) % 64 != 0 and len(p) % 64 != 0
    return p, tri, dict((flags, rc.repair(p, tri, flags)) for flags in FLAGS)


@pytest.mark.parametrize("flags", FLAGS)
def test_many_tiles(ctx, big_torus, flags):
    p, tri, wants = big_torus
    want = check(ctx, p, tri, flags, wants[flags])
    assert want[2]["droppedTriangles"] == 320 and want[2]["repeatedSides"] == 416
    assert want[2]["splitVertices"] == (64 if flags else 0)
    assert manifold(ctx, p, tri)["manifold"] == 0 and manifold(ctx, want[0], want[1])["manifold"] == 1


# ---------------------------------------------------------------- one hub

@pytest.mark.parametrize("flags", FLAGS)
def test_one_hub(ctx, flags):
    """Two cones of 10 000 triangles on one hub of degree 20 000, in the middle of the numbering: whole waves of records share
    one of two roots, and the two groups are numbered between their neighbours."""
    p, tri = rc.bowtie(10_000, 10_000, hub=7777)
    want = check(ctx, p, tri, flags)
    assert (want[2]["splitVertices"], want[2]["addedVertices"], want[2]["outVertices"]) == (1, 1, 20_002)
    assert want[3][7776:7780].tolist() == [7776, 7777, 7777, 7778]
    # two chains and a ring on hub 15 000, and vertices that nothing uses
    mixed = np.concatenate([rc.fan(5_000, 15_000, 0), tc.cone(3_000, 15_000, 10_001), rc.fan(4_000, 15_000, 6_000)])
    want = check(ctx, rc.positions(15_001, 5), mixed, flags)
    assert (want[2]["splitVertices"], want[2]["addedVertices"], want[2]["unusedVertices"]) == (1, 2 if flags else 1, 999 + 1_999)
    assert want[3][-3:].tolist() == [15_000] * 3 if flags else want[3][-2:].tolist() == [15_000] * 2


# ---------------------------------------------------------------- beyond the one-launch scan

def test_beyond_the_one_launch_scans(ctx):
    """The scan over the records that numbers the output vertices: more than 1 024 tiles of 2 048 take the two-launch form,
    which evaluates its input functor twice.  A grid of 3 T = 2 095 302 records, and behind it a hundred small defective meshes
    whose records lie on both sides of record 2 097 152."""
    p, tri = rc.grid_mesh(600, 584)
    assert 3 * len(tri) == 2_095_302
    ps, ts, base = [p], [tri], len(p)
    for k in range(100):
        for q, t in (rc.bowtie(4, 5, hub=k % 10), rc.cone_and_fan(), rc.twice(3, 4)):
            ps.append(q.astype(np.float32) + np.float32(1000 + k))
            ts.append(t + base)
            base += len(q)
    p, tri = np.concatenate(ps).astype(np.float32), np.concatenate(ts)
    assert 3 * len(tri) > 1024 * 2048 + 4096 and (tri[:698_434] < 600 * 584).all()
    for flags in FLAGS:
        want = check(ctx, p, tri, flags)
        assert (want[2]["splitVertices"], want[2]["droppedTriangles"], want[2]["repeatedSides"]) == (200, 200, 600)
        first_new = int(np.flatnonzero(want[3] >= 600 * 584)[0])
        assert first_new == 600 * 584 and want[2]["outVertices"] == len(p) + 200


# ---------------------------------------------------------------- capacities and guard bands

@pytest.mark.parametrize("with_source", [False, True])
def test_capacities_and_guard_bands(ctx, with_source):
    from mlsgpu_amd import binding as b
    p, tri = rc.simplified_torus(97, 61, 0.125, 0.11)
    want = rc.repair(p, tri, rc.SPLIT_PINCHES)
    V, T, V2, T2, G = len(p), len(tri), want[2]["outVertices"], want[2]["outTriangles"], 1024
    assert want[2]["addedVertices"] == 17 and T2 == T - 70
    dv, dt = b.DeviceBuffer(ctx, array=p), b.DeviceBuffer(ctx, array=tri.astype(np.uint32))
    band_v, band_t = np.full(2 * G + 3 * V2, -123.25, np.float32), np.full(2 * G + 3 * T2, 0xDEADBEEF, np.uint32)
    band_s = np.full(2 * G + V2, 0xFEEDFACE, np.uint32)
    ov, ot, os_ = b.DeviceBuffer(ctx, array=band_v), b.DeviceBuffer(ctx, array=band_t), b.DeviceBuffer(ctx, array=band_s)

    def call(cap_v, cap_t, with_outputs=True):
        st = b.RepairStats()
        code = b.lib().mlsgpu_hip_mesh_repair(ctx.h, dv.ptr, V, dt.ptr, T, rc.SPLIT_PINCHES, ov.ptr + 4 * G if with_outputs else None, cap_v,
                                              ot.ptr + 4 * G if with_outputs else None, cap_t,
                                              os_.ptr + 4 * G if with_outputs and with_source else None, C.byref(st))
        return code, st.as_dict()

    def untouched():
        return (ov.download(np.float32).tobytes() == band_v.tobytes() and ot.download(np.uint32).tobytes() == band_t.tobytes()
                and os_.download(np.uint32).tobytes() == band_s.tobytes())

    assert call(0, 0, with_outputs=False) == (2, want[2])           # the size query
    assert b"the repaired mesh has" in b.lib().mlsgpu_hip_last_error()
    assert call(V2 - 1, T2) == (2, want[2]) and untouched()         # one short in vertices
    assert call(V2, T2 - 1) == (2, want[2]) and untouched()         # one short in triangles
    code, st = call(V2, T2)
    assert code == 0
    got_v, got_t, got_s = ov.download(np.float32), ot.download(np.uint32), os_.download(np.uint32)
    assert (got_v[:G] == -123.25).all() and (got_v[G + 3 * V2:] == -123.25).all()
    assert (got_t[:G] == 0xDEADBEEF).all() and (got_t[G + 3 * T2:] == 0xDEADBEEF).all()
    assert (got_s[:G] == 0xFEEDFACE).all() and (got_s[G + V2:] == 0xFEEDFACE).all()
    if with_source:
        rc.assert_same((got_v[G:G + 3 * V2], got_t[G:G + 3 * T2], st, got_s[G:G + V2]), want)
    else:
        rc.assert_same((got_v[G:G + 3 * V2], got_t[G:G + 3 * T2], st), want)
        assert got_s.tobytes() == band_s.tobytes()
    assert dv.download(np.float32).tobytes() == p.tobytes()         # the inputs are left alone
    assert dt.download(np.uint32).tobytes() == tri.astype(np.uint32).tobytes()
    for buf in (dv, dt, ov, ot, os_):
        buf.free()


# ---------------------------------------------------------------- errors

def small_correct_call(ctx):
    check(ctx, *rc.fin(5, 6), rc.SPLIT_PINCHES)


def test_errors_leave_the_context_usable(ctx):
    import mlsgpu_amd as m
    from mlsgpu_amd import binding as b
    p, tri = rc.bowtie()
    for flags in (2, 3, 1 << 31):
        with pytest.raises(rc.Invalid):
            rc.repair(p, tri, flags)
        with pytest.raises(b.InvalidArgument):
            run(ctx, p, tri, flags)
        small_correct_call(ctx)
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st = b.RepairStats()
    for num_triangles, num_vertices in ((1, 2 ** 32), ((2 ** 32 + 2) // 3, 10)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_repair(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, 0, None, 0, None, 0, None,
                                                   C.byref(st)))
    with pytest.raises(b.InvalidArgument):
        b.check(b.lib().mlsgpu_hip_mesh_repair(ctx.h, one.ptr, 1, one.ptr, 1, 0, None, 0, None, 0, None, None))
    one.free()
    small_correct_call(ctx)
    mesher = m.Mesher(ctx, 0.02)
    with pytest.raises(b.InvalidArgument):
        mesher.repair()                                             # before finalize
    mesher.close()
    small_correct_call(ctx)


# ---------------------------------------------------------------- determinism

@pytest.mark.parametrize("flags", FLAGS)
def test_determinism(ctx, big_torus, flags):
    p, tri, wants = big_torus
    want = wants[flags]
    runs = [run(ctx, p, tri, flags) for _ in range(3)]
    for r in runs:
        assert r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes() and r[2] == runs[0][2]
        assert r[3].tobytes() == runs[0][3].tobytes()
    rc.assert_same(runs[0], want)
    rng = np.random.default_rng(3)
    order = rng.permutation(len(tri))                               # permuted triangles: only the output triangles move
    v, t, st, src = run(ctx, p, tri[order], flags)
    assert st == want[2] and v.tobytes() == want[0].tobytes() and src.tobytes() == want[3].tobytes()
    assert sc.canonical(t) == sc.canonical(want[1])
    rc.assert_same((v, t, st, src), rc.repair(p, tri[order], flags))
    small = rc.simplified_torus(97, 61, 0.125, 0.11)                # renumbered vertices: the same soup
    soup = rc.soup(*check(ctx, *small, flags)[:2])
    q, qtri, _ = rc.renumbered(*small, 4)
    v, t, st, _ = check(ctx, q, qtri, flags)
    assert st["droppedTriangles"] == 70 and rc.soup(v, t) == soup


# ---------------------------------------------------------------- simplify -> repair -> fill holes

@pytest.mark.parametrize("flags", FLAGS)
def test_chain_with_simplify_and_fill_holes(ctx, flags):
    """What the stage is for: the device's own simplify makes a torus non-manifold, the repair makes it manifold again, and the
    hole filling -- which leaves irregular boundaries alone -- then closes what the dropped triangles left."""
    from mlsgpu_amd import binding as b
    p, tri = rc.torus_mesh(200, 90, 0.5, 0.05)
    v, t, _ = b.mesh_simplify(ctx, p, tri.astype(np.uint32), (-1.0, -1.0, -1.0), 0.06)
    assert manifold(ctx, v, t)["count"][tc.DUPLICATED] == 33
    want = check(ctx, v, t, flags)
    repaired = manifold(ctx, want[0], want[1])
    assert repaired["manifold"] == 1 and repaired["numBoundaries"] == 11
    fv, ft, fs = b.mesh_fill_holes(ctx, want[0], want[1], 32)
    fc.assert_same((fv, ft, fs), fc.fill(want[0], want[1], 32))
    filled = manifold(ctx, fv, ft)
    assert filled["manifold"] == 1 and filled["numBoundaries"] == (0 if flags else 9)
    assert fs["irregularEdges"] == (0 if flags else 97)             # split pinches: every boundary is regular, and filled


# ---------------------------------------------------------------- the device sink

def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def summed(stats):
    return dict((name, sum(st[name] for st in stats)) for name in rc.STAT_NAMES)


@pytest.mark.parametrize("chunks", [1, 2])
def test_sink(ctx, tmp_path, chunks):
    """One bucket in one chunk, eight buckets in two, finalized and simplified in cells of 2.5 grid spacings -- of the cells
    2, 2.5, 3, 3.5, 4 and 5 the smallest at which the simplify oracle leaves every one of these chunks non-manifold: each
    repaired chunk is the oracle's for its own earlier download; normals, files and the topology report follow the repaired
    chunks; a finalize brings the chunks back."""
    from mlsgpu_amd import binding as b
    from test_gpu_simplify import filled_sink
    CELL, ORIGIN = 2.5, (-2.5, -2.5, -2.5)
    mesher, buckets = filled_sink(ctx, 47, lambda k: 0) if chunks == 1 else filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    with pytest.raises(b.InvalidArgument):
        mesher.repair()                                             # before finalize
    assert buckets == (1 if chunks == 1 else 8) and mesher.finalize() == chunks
    original = [mesher.chunk(i) for i in range(chunks)]
    finalize_stats = mesher.stats()
    mesher.simplify(ORIGIN, CELL)
    before = [mesher.chunk(i) for i in range(chunks)]
    assert all(tc.report_fields(mesher.chunk_topology(i))["count"][tc.DUPLICATED] > 0 for i in range(chunks))
    mesher.chunk_normals(0)                                         # computed before the call: must not be served after it
    for flags in FLAGS:                                             # the second round runs on the first one's chunks
        want = [rc.repair(c["vertices"], c["triangles"], flags) for c in before]
        st = mesher.repair(flags)
        print("sink chunks %d flags %d: %s" % (chunks, flags, st))
        assert st == summed([w[2] for w in want]) and mesher.stats() == finalize_stats
        assert (st["droppedTriangles"] > 0) == (flags == 0) and (st["splitVertices"] > 0) == (flags != 0)
        for i in range(chunks):
            c = mesher.chunk(i)
            assert len(c["triangles"]) > 100 and c["chunk"] == before[i]["chunk"]
            rc.assert_same((c["vertices"], c["triangles"], want[i][2]), want[i])
            report = tc.report_fields(mesher.chunk_topology(i))
            assert report == tc.count_all(len(want[i][0]), want[i][1]) and report["manifold"] == 1
            got = mesher.chunk_normals(i)
            nc.assert_same((got["normals"], got["stats"]), nc.normals(want[i][0], want[i][1]))
            mesher.write_ply(i, tmp_path / "device.ply", comments=("c",))
            b.write_ply(tmp_path / "host.ply", want[i][0], want[i][1], comments=("c",))
            assert file_bytes(tmp_path / "device.ply") == file_bytes(tmp_path / "host.ply")
        with pytest.raises(b.InvalidArgument):
            mesher.repair(2)                                        # a refused parameter costs no results
        assert mesher.chunk(0)["triangles"].tobytes() == want[0][1].tobytes()
        again = mesher.repair(flags)                                # it may be called again, and changes nothing then
        assert again == summed([dict(rc.repair(w[0], w[1], flags)[2]) for w in want])
        assert again["outVertices"] == st["outVertices"] and again["droppedTriangles"] == again["addedVertices"] == 0
        for i in range(chunks):
            c = mesher.chunk(i)
            assert c["vertices"].tobytes() == want[i][0].tobytes() and c["triangles"].tobytes() == want[i][1].tobytes()
        before = [mesher.chunk(i) for i in range(chunks)]
    total = sum(len(c["triangles"]) for c in before)
    assert mesher.fill_holes(32)["numTriangles"] == total           # fill holes, smooth and simplify work on the repaired chunks
    filled = sum(mesher.chunk(i)["num_triangles"] for i in range(chunks))
    assert mesher.smooth(2)["numTriangles"] == filled
    assert mesher.simplify(ORIGIN, 2 * CELL)["inTriangles"] == filled
    assert mesher.finalize() == chunks                              # finalize again: the chunks as they were
    for i in range(chunks):
        c = mesher.chunk(i)
        assert c["vertices"].tobytes() == original[i]["vertices"].tobytes() and c["triangles"].tobytes() == original[i]["triangles"].tobytes()
    mesher.close()


# ---------------------------------------------------------------- reconstruct --repair

# On the mesh that the command below writes without --simplify, the simplify oracle at 1, 1.25, 1.5 ... grid spacings (origin
# one cell below the grid's low corner, as reconstruct places it) gives a manifold mesh at 1 and 132 DUPLICATED vertices at
# 1.25: the smallest cell of this search at which `--simplify N --check` prints `manifold no`.
SIMPLIFY = "1.25"


def test_reconstruct_repair(ctx, tmp_path):
    """examples/reconstruct --simplify 1.25 --repair --check: one more line, `manifold yes` for every chunk, and a file that is the
    oracle's for the file the same command writes without --repair (a simplified mesh does not depend on the order in which the
    worker threads deliver, so the two runs can be compared index by index)."""
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

    head = [exe, "--weld", "device", "--simplify", SIMPLIFY]
    plain = subprocess.check_output(head + ["--check"] + args("plain.ply"), timeout=300).decode().splitlines()
    print("\n".join(plain))
    assert len(plain) == 3 and plain[2].startswith("topology chunk 0 manifold no"), plain
    V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
    assert tc.count_all(len(V), tri)["manifold"] == 0
    for option, flags in ((["--repair"], 0), (["--repair", "pinches"], rc.SPLIT_PINCHES)):
        out = subprocess.check_output(head + option + ["--check"] + args("out.ply"), timeout=300).decode().splitlines()
        print("\n".join(out))
        assert len(out) == 4 and out[:2] == plain[:2], out
        assert all(line.startswith("topology chunk") and " manifold yes " in line for line in out[3:])
        line = re.fullmatch(r"repair chunks (\d+) out-of-range (\d+) degenerate (\d+) repeated-sides (\d+) dropped (\d+) unused (\d+) "
                            r"split (\d+) vertices (\d+) -> (\d+) triangles (\d+) -> (\d+)", out[2])
        assert line, out[2]
        wantV, wantT, st, _ = rc.repair(V, tri, flags)
        assert [int(x) for x in line.groups()] == [1, st["outOfRangeTriangles"], st["degenerateTriangles"], st["repeatedSides"],
                                                   st["droppedTriangles"], st["unusedVertices"], st["splitVertices"], len(V),
                                                   st["outVertices"], len(tri), st["outTriangles"]]
        assert st["droppedTriangles"] > 0
        gotV, gotT = parse_ply_mesh(str(tmp_path / "out.ply"))
        rc.assert_same((gotV, gotT, st), (wantV, wantT, st))
        report = tc.count_all(len(gotV), gotT)
        assert report["manifold"] == 1
        assert re.search(r" components %d boundaries %d " % (report["numComponents"], report["numBoundaries"]), out[3])
    refused = subprocess.run([exe, "--weld", "host", "--repair"] + args("host.ply"), capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--repair needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
