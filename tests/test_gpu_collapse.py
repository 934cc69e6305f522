"""The device short-edge collapse (mlsgpu_hip_mesh_collapse_edges, mlsgpu_hip_mesher_collapse_edges, reconstruct
--collapse-edges) against the CPU oracle of collapse_cases.py: every vertex bit, every triangle row, every source index and every
statistic.  test_collapse_oracle.py checks on the CPU that the inputs used here converge within MAX_ROUNDS."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import collapse_cases as cc
import flip_cases as fc
import normals_cases as nc
import smooth_cases as sc
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_ROUNDS = 64
SINK_LENGTH = 0.3               # of the sink's grid spacing of 1


def rows32(triangles):
    return (np.asarray(triangles, np.int64) & 0xFFFFFFFF).astype(np.uint32)


def run(ctx, vertices, triangles, max_length, max_rounds=MAX_ROUNDS, min_cos=cc.MIN_COS):
    from mlsgpu_amd import binding as b
    return b.mesh_collapse_edges(ctx, vertices, rows32(triangles), max_rounds, max_length, min_cos, with_source=True)


def check(ctx, vertices, triangles, max_length, max_rounds=MAX_ROUNDS, min_cos=cc.MIN_COS):
    want = cc.collapse(vertices, triangles, max_rounds, max_length, min_cos)
    cc.assert_same(run(ctx, vertices, triangles, max_length, max_rounds, min_cos), want)
    return want


# ---------------------------------------------------------------- hand cases and empty meshes

def test_hand_cases(ctx):
    v, t, st, src = check(ctx, *cc.disk(), 0.05)
    assert (st["collapses"], st["rounds"], st["converged"], len(v), len(t)) == (1, 2, 1, 17, 24) and v[0].tolist() == [0, 0, 0]
    assert src.tolist() == [0] + list(range(2, 18))
    p, tri = cc.disk(rim=True)
    v, t, st, src = check(ctx, p, tri, 0.05)
    assert st["collapses"] == 1 and src.tolist() == list(range(1, 10)) and v[0].tobytes() == p[1].tobytes()
    for build, length, short in ((fc.kite, 10.0, 1), (fc.tetrahedron, 100.0, 6), (cc.tube, 0.05, 12), (cc.star, 0.012, 1)):
        st = check(ctx, *build(), length)[2]
        assert (st["shortBefore"], st["blockedAfter"], st["collapses"], st["rounds"], st["converged"]) == (short, short, 0, 1, 1)
    assert check(ctx, *cc.star(), 0.012, min_cos=0.0)[2]["blockedAfter"] == 1       # it would turn over, not only tilt
    assert check(ctx, *cc.coincident(), 0.0)[2]["collapses"] == 1
    for build in (cc.disk, fc.kite, fc.tetrahedron, fc.pillow, cc.tube, cc.star, cc.coincident):
        for length, min_cos in ((0.05, 0.5), (100.0, 0.0), (100.0, 1.0)):
            for rounds in (0, 1, MAX_ROUNDS):
                check(ctx, *build(), length, rounds, min_cos)
    p, tri = cc.needle_row()
    assert check(ctx, p, tri, 0.05, 3)[2]["converged"] == 0
    st = check(ctx, p, tri, 0.05)[2]
    assert st["converged"] == 1 and st["rounds"] > 8 and st["shortAfter"] == 0


def test_empty_meshes_and_pure_report(ctx):
    p, tri = fc.flat_grid(4, 4, 0.3, 1)
    v, t, st, _ = check(ctx, p, tri, 0.5, 0)                        # maxRounds = 0: a pure report, the output a copy
    assert v.tobytes() == p.tobytes() and t.tolist() == tri.tolist() and st["numEdges"] == 33 and st["qualityBefore"] == st["qualityAfter"]
    none = dict(cc.empty_stats(), rounds=1, converged=1)            # no triangle takes part: the first round finds no winner
    assert check(ctx, p[:0], tri[:0], 0.5)[2] == none and check(ctx, p[:0], tri[:0], 0.5, 0)[2] == cc.empty_stats()
    v, t, st, _ = check(ctx, p, tri[:0], 0.5)                       # T = 0: every vertex is unused
    assert len(v) == 0 and len(t) == 0 and st == dict(none, numVertices=16, unusedVertices=16)
    assert check(ctx, p, tri[:0], 0.5, 0)[2]["rounds"] == 0
    v, t, st, _ = check(ctx, p[:0], tri, 0.5)                       # V = 0: every index is out of range
    assert len(t) == 0 and st == dict(none, numTriangles=18, outOfRangeTriangles=18)


def test_classification_order(ctx):
    """An index >= V wins over a vertex twice, as for the flips; neither is part of the output."""
    import topology_cases as tc
    p, tri = tc.classification_trap()
    _, t, st, _ = check(ctx, p, tri, 0.0)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["numEdges"], st["interiorEdges"]) == (2, 1, 5, 1)
    assert len(t) == len(tri) - 3


# ---------------------------------------------------------------- grids

def test_planted_needles(ctx):
    st = check(ctx, *cc.planted_needles(), 0.05)[2]
    assert st["collapses"] == 64 and st["minQualityBefore"] < 1e-3 and st["minQualityAfter"] > 0.2


def test_jittered_grids(ctx):
    st = check(ctx, *fc.grid_mesh(40, 40, jitter=0.45, seed=2), 0.5)[2]
    assert (st["collapses"], st["rounds"], st["converged"]) == (75, 6, 1)
    st = check(ctx, *fc.flat_grid(40, 40, 0.45, 1), 0.5)[2]
    assert (st["collapses"], st["rounds"], st["converged"]) == (145, 8, 1) and st["shortAfter"] == st["blockedAfter"] == 4
    for rounds in (0, 1, 3):                                        # the cap on the rounds
        assert check(ctx, *fc.flat_grid(40, 40, 0.45, 1), 0.5, rounds)[2]["converged"] == 0
    check(ctx, *fc.flat_grid(40, 40, 0.45, 1), 0.5, MAX_ROUNDS, 1.0)       # minCos 1 blocks what is not flat to the bit
    check(ctx, *fc.grid_mesh(40, 40, jitter=0.45, seed=2), 0.7, MAX_ROUNDS, 0.0)


@pytest.fixture(scope="module")
def big_grid():
    p, tri = fc.grid_mesh(300, 300, jitter=0.3, seed=11)
    assert p.shape == (90_000, 3) and tri.shape == (178_802, 3)
    return p, tri, cc.collapse(p, tri, MAX_ROUNDS, 0.5)


def test_several_sort_tiles(ctx, big_grid):
    p, tri, want = big_grid
    cc.assert_same(run(ctx, p, tri, 0.5), want)
    assert want[2]["converged"] == 1 and want[2]["collapses"] > 400 and want[2]["rounds"] > 2
    assert 3 * len(tri[:-1]) % 64 != 0 and len(tri[:-1]) % 64 != 0 and len(p) % 64 != 0       # a partial last wave
    check(ctx, p, tri[:-1], 0.5)


# ---------------------------------------------------------------- one hub

def test_fan_around_one_hub(ctx):
    """One hub of valence 20 000 inside a fixed rim: every spoke is short and blocked by the valence cap before anything
    walks the hub's segment, and one classification suffices."""
    p, tri = nc.fan_mesh(20_000, seed=1)
    st = check(ctx, p, tri, 10.0)[2]
    assert (st["interiorEdges"], st["shortBefore"], st["blockedAfter"], st["rounds"], st["converged"]) == (20_000, 20_000, 20_000, 1, 1)
    assert st["fixedVertices"] == 20_000 and st["collapses"] == 0


# ---------------------------------------------------------------- closed surface, scaling

def test_closed_torus_and_scaling(ctx):
    from mlsgpu_amd import binding as b
    import topology_cases as tc
    p, tri = sc.noisy_torus(200, 40, 0.004, 7)
    v, t, st, src = check(ctx, p, tri, 0.01)
    assert st["converged"] == 1 and st["collapses"] > 100 and st["fixedVertices"] == 0 and st["numEdges"] == st["interiorEdges"] == 24_000
    keep = ("manifold", "numComponents", "numBoundaries", "boundaryEdges", "eulerCharacteristic")
    before, after = tc.report_fields(b.mesh_topology(ctx, rows32(tri), len(p))), tc.report_fields(b.mesh_topology(ctx, t, len(v)))
    assert before["manifold"] == 1 and [after[k] for k in keep] == [before[k] for k in keep]
    for shift in (-7, 40, -60):
        s = np.float32(2.0) ** np.float32(shift)
        got = run(ctx, p * s, tri, 0.01 * float(s))
        want = dict(st, minLengthSqBefore=st["minLengthSqBefore"] * float(s) ** 2, minLengthSqAfter=st["minLengthSqAfter"] * float(s) ** 2)
        cc.assert_same(got, (v * s, t, want, src))


# ---------------------------------------------------------------- counters, guard bands

def test_counters_guard_bands_and_size_query(ctx):
    from mlsgpu_amd import binding as b
    p, tri = cc.defect_mesh()
    assert (tri == 0xFFFFFFFF).sum() == 1
    want = check(ctx, p, tri, 0.6)
    st = want[2]
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 2) and st["collapses"] > 3
    assert st["unusedVertices"] == 2 + st["collapses"] and st["outTriangles"] == len(tri) - 4 - 2 * st["collapses"]
    nv, nt, G = st["outVertices"], st["outTriangles"], 1024
    rows = rows32(tri)
    dv, dt = b.DeviceBuffer(ctx, array=p), b.DeviceBuffer(ctx, array=rows)
    got = b.CollapseStats()
    args = (ctx.h, dv.ptr, len(p), dt.ptr, len(tri), MAX_ROUNDS, 0.6, cc.MIN_COS)
    with pytest.raises(b.LengthError, match="the result has %d and %d" % (nv, nt)):        # the size query: complete statistics
        b.check(b.lib().mlsgpu_hip_mesh_collapse_edges(*args, None, 0, None, 0, None, C.byref(got)))
    assert got.as_dict() == st
    outs = [b.DeviceBuffer(ctx, array=np.full(2 * G + words, 0xABCD1234, np.uint32)) for words in (3 * nv, 3 * nt, nv)]
    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1)):               # one row short: nothing is written
        with pytest.raises(b.LengthError):
            b.check(b.lib().mlsgpu_hip_mesh_collapse_edges(*args, outs[0].ptr + 4 * G, cap_v, outs[1].ptr + 4 * G, cap_t, outs[2].ptr + 4 * G,
                                                           C.byref(got)))
        assert all((o.download(np.uint32) == 0xABCD1234).all() for o in outs)
    b.check(b.lib().mlsgpu_hip_mesh_collapse_edges(*args, outs[0].ptr + 4 * G, nv, outs[1].ptr + 4 * G, nt, outs[2].ptr + 4 * G, C.byref(got)))
    bands = [o.download(np.uint32) for o in outs]
    assert all((x[:G] == 0xABCD1234).all() and (x[-G:] == 0xABCD1234).all() for x in bands)
    cc.assert_same((bands[0][G:-G].view(np.float32), bands[1][G:-G], got.as_dict(), bands[2][G:-G]), want)
    assert dt.download(np.uint32).tobytes() == rows.tobytes()       # the inputs are left alone
    assert dv.download(np.float32).tobytes() == p.tobytes()
    for buf in [dv, dt] + outs:
        buf.free()


# ---------------------------------------------------------------- determinism

def test_determinism(ctx, big_grid):
    p, tri, want = big_grid
    a, b = run(ctx, p, tri, 0.5), run(ctx, p, tri, 0.5)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))) and a[2] == b[2]
    order = np.random.default_rng(3).permutation(len(tri))          # a permutation of the triangles: the same vertices and set
    got = run(ctx, p, tri[order], 0.5)
    assert got[2] == want[2] and got[0].tobytes() == want[0].tobytes() and got[3].tolist() == want[3].tolist()
    assert cc.triangle_set(got[1]).tolist() == cc.triangle_set(want[1]).tolist()
    turns = np.random.default_rng(4).integers(0, 3, len(tri))       # rotated corners: the same again
    turned = np.stack([tri[np.arange(len(tri)), (turns + k) % 3] for k in range(3)], axis=1)
    got = run(ctx, p, turned, 0.5)
    assert got[0].tobytes() == want[0].tobytes() and cc.triangle_set(got[1]).tolist() == cc.triangle_set(want[1]).tolist()
    assert dict(got[2], **QUALITY_OF(want[2])) == want[2]
    p, tri = fc.flat_grid(40, 40, 0.45, 1)                          # free of ties: renumbering the vertices renumbers the result
    want = cc.collapse(p, tri, MAX_ROUNDS, 0.5)
    q, qtri, perm = cc.renumbered(p, tri, 5)
    got = run(ctx, q, qtri, 0.5)
    assert dict(got[2], **QUALITY_OF(want[2])) == want[2]
    # the same positions; of two free ends the smaller number survives, so the sources need not be perm's images
    assert sorted(map(bytes, got[0].view("V12").ravel())) == sorted(map(bytes, want[0].view("V12").ravel()))


def QUALITY_OF(stats):
    """The quality report's fields: q is computed on a triangle's corners in row order, so rotating them may move its last bit."""
    return dict((k, stats[k]) for k in ("minQualityBefore", "minQualityAfter", "qualityBefore", "qualityAfter"))


# ---------------------------------------------------------------- errors

def small_correct_call(ctx):
    check(ctx, *fc.flat_grid(9, 11, 0.45, 3), 0.5)


def test_errors_leave_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    p, tri = fc.flat_grid(9, 11, 0.3, 3)
    p[40, 1] = np.nan
    p[60, 0] = np.inf
    with pytest.raises(cc.Invalid, match="vertex"):
        cc.collapse(p, tri, 2, 0.5)
    with pytest.raises(b.InvalidArgument, match="2 vertices have a coordinate that is not finite"):
        run(ctx, p, tri, 0.5, 2)
    with pytest.raises(b.InvalidArgument, match="2 vertices have a coordinate that is not finite"):
        run(ctx, p, tri[:0], 0.5, 2)
    small_correct_call(ctx)
    p, tri = cc.disk()
    for max_length, min_cos in [(-1e-9, 0.5), (np.inf, 0.5), (np.nan, 0.5), (0.1, 1.5), (0.1, -0.5), (0.1, np.nan)]:
        with pytest.raises(cc.Invalid, match="parameters"):
            cc.collapse(p, tri, 1, max_length, min_cos)
        with pytest.raises(b.InvalidArgument):
            run(ctx, p, tri, max_length, 1, min_cos)
        small_correct_call(ctx)
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    with pytest.raises(b.InvalidArgument):
        b.check(b.lib().mlsgpu_hip_mesh_collapse_edges(ctx.h, one.ptr, 1, one.ptr, 1, 1, 0.1, 0.5, one.ptr, 1, one.ptr, 1, None, None))
    st = b.CollapseStats()
    for num_triangles, num_vertices in ((1, 2 ** 32), ((2 ** 32 + 2) // 3, 10)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(b.lib().mlsgpu_hip_mesh_collapse_edges(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, 1, 0.1, 0.5, one.ptr, 1,
                                                           one.ptr, 1, None, C.byref(st)))
    one.free()
    small_correct_call(ctx)


# ---------------------------------------------------------------- the device sink

def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def summed(stats):
    out = dict((name, sum(st[name] for st in stats)) for name in cc.STAT_NAMES if not name.startswith(("min", "quality")))
    out["rounds"] = max(st["rounds"] for st in stats)
    out["converged"] = min(st["converged"] for st in stats)
    for name in ("minQualityBefore", "minQualityAfter", "minLengthSqBefore", "minLengthSqAfter"):
        out[name] = min(st[name] for st in stats)
    for name in ("qualityBefore", "qualityAfter"):
        out[name] = [sum(st[name][k] for st in stats) for k in range(16)]
    return out


@pytest.mark.parametrize("chunks", [1, 2])
def test_sink(ctx, tmp_path, chunks):
    """One bucket in one chunk, eight buckets in two: each chunk is the oracle's for its own earlier download, the seam's
    vertices and edges stay, the topology report's invariants stay, normals and files follow the new chunk, a finalize brings
    the chunks back."""
    import topology_cases as tc
    from mlsgpu_amd import binding as b
    from test_gpu_flip import seam_edges, summed as flips_summed
    from test_gpu_simplify import filled_sink
    from test_gpu_smooth import rows_of
    mesher, buckets = filled_sink(ctx, 47, lambda k: 0) if chunks == 1 else filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    with pytest.raises(b.InvalidArgument):
        mesher.collapse_edges(MAX_ROUNDS, SINK_LENGTH)              # before finalize
    assert buckets == (1 if chunks == 1 else 8) and mesher.finalize() == chunks
    before = [mesher.chunk(i) for i in range(chunks)]
    keep = ("manifold", "numComponents", "numBoundaries", "boundaryEdges", "eulerCharacteristic")
    topology = [tc.report_fields(mesher.chunk_topology(i)) for i in range(chunks)]
    shared = rows_of(before[0]["vertices"]) & rows_of(before[-1]["vertices"]) if chunks == 2 else set()
    seams = [seam_edges(c, shared) for c in before]
    assert chunks == 1 or (len(shared) > 100 and all(len(s) > 50 for s in seams))
    mesher.chunk_normals(0)                                         # computed before the call: must not be served after it
    want = [cc.collapse(c["vertices"], c["triangles"], MAX_ROUNDS, SINK_LENGTH) for c in before]
    st = mesher.collapse_edges(MAX_ROUNDS, SINK_LENGTH)
    print("sink", chunks, dict((k, st[k]) for k in ("collapses", "rounds", "shortBefore", "blockedAfter", "minQualityBefore", "minQualityAfter")))
    assert st == summed([w[2] for w in want]) and st["converged"] == 1 and st["collapses"] > 100
    for i in range(chunks):
        c = mesher.chunk(i)
        assert len(c["triangles"]) > 1000 and c["chunk"] == before[i]["chunk"]
        cc.assert_same((c["vertices"], c["triangles"], want[i][2]), want[i])
        after = tc.report_fields(mesher.chunk_topology(i))
        assert [after[k] for k in keep] == [topology[i][k] for k in keep]
        assert shared <= rows_of(c["vertices"]) and seam_edges(c, shared) == seams[i]      # the seam is as it was
        got = mesher.chunk_normals(i)
        nc.assert_same((got["normals"], got["stats"]), nc.normals(c["vertices"], want[i][1]))
        mesher.write_ply(i, tmp_path / "device.ply", comments=("c",))
        b.write_ply(tmp_path / "host.ply", want[i][0], want[i][1], comments=("c",))
        assert file_bytes(tmp_path / "device.ply") == file_bytes(tmp_path / "host.ply")
    with pytest.raises(b.InvalidArgument):
        mesher.collapse_edges(MAX_ROUNDS, SINK_LENGTH, min_cos=2.0)         # a refused parameter costs no results
    again = mesher.collapse_edges(MAX_ROUNDS, SINK_LENGTH)          # it may be called again: a fixed point
    assert (again["collapses"], again["rounds"], again["shortBefore"], again["unusedVertices"]) == (0, 1, st["shortAfter"], 0)
    flips = [fc.flip(w[0], w[1], MAX_ROUNDS) for w in want]        # the flips work on the new chunks
    assert mesher.flip_edges(MAX_ROUNDS) == flips_summed([f[1] for f in flips])
    for i in range(chunks):
        c = mesher.chunk(i)
        fc.assert_same((c["triangles"], flips[i][1]), flips[i])
        assert c["vertices"].tobytes() == want[i][0].tobytes()
    assert mesher.finalize() == chunks                              # finalize again: the chunks as they were
    for i in range(chunks):
        c = mesher.chunk(i)
        assert c["vertices"].tobytes() == before[i]["vertices"].tobytes() and c["triangles"].tobytes() == before[i]["triangles"].tobytes()
    mesher.close()


# ---------------------------------------------------------------- reconstruct --collapse-edges

def test_reconstruct_collapse_edges(ctx, tmp_path):
    """examples/reconstruct --collapse-edges 0.3: one more line, and a file that is a converged collapse of the file the same
    command writes without the option.  Two runs number their vertices in the order their worker threads deliver, and
    marching's lattice makes edges of exactly equal length, whose tie the vertex numbers break: the two files are compared
    through everything that does not depend on a tie (test_sink compares every bit, within one run).  Collapse comes before
    --flip-edges when both are given; refused for the host welder."""
    from test_gpu_smooth import rows_of
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

    pattern = (r"collapse-edges chunks (\d+) interior-edges (\d+) fixed (\d+) rounds (\d+) collapses (\d+) short (\d+) -> (\d+) "
               r"blocked (\d+) vertices (\d+) -> (\d+) triangles (\d+) -> (\d+) min-quality ([-+0-9.e]+) -> ([-+0-9.e]+)")
    plain = reconstruct("plain.ply")
    out = reconstruct("out.ply", "--collapse-edges", "0.3")
    assert len(out) == len(plain) + 1 and out[:-1] == plain, out
    V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
    gotV, gotT = parse_ply_mesh(str(tmp_path / "out.ply"))
    st = cc.collapse(V, tri, 0, 0.3, 0.5)[2]                        # what the input's report says whatever the numbering
    line = re.fullmatch(pattern, out[-1])
    assert line, out[-1]
    (chunks, interior, fixed, rounds, collapses, short_before, short_after, blocked, v_in, v_out, t_in, t_out) = [int(x) for x in line.groups()[:12]]
    assert (chunks, interior, fixed, short_before, v_in, t_in) == (1, st["interiorEdges"], st["fixedVertices"], st["shortBefore"], len(V), len(tri))
    assert float(line.group(13)) == float("%.9g" % st["minQualityBefore"])
    assert collapses > 1000 and 1 < rounds <= 64 and short_after == blocked < short_before
    assert (v_out, t_out) == (v_in - collapses, t_in - 2 * collapses) == (len(gotV), len(gotT))
    again = cc.collapse(gotV, gotT, 64, 0.3, 0.5)[2]                # the file is a fixed point with the line's leftovers and quality
    assert (again["collapses"], again["shortBefore"], again["blockedAfter"], again["unusedVertices"]) == (0, short_after, blocked, 0)
    assert float(line.group(14)) == float("%.9g" % again["minQualityBefore"])
    assert cc.invariants(len(gotV), gotT) == cc.invariants(len(V), tri)
    sides = set(map(tuple, np.stack([tri.ravel(), tri[:, [1, 2, 0]].ravel()], axis=1).tolist()))
    rim = sorted(set(x for a, b in sides if (b, a) not in sides for x in (a, b)))
    assert len(rim) == fixed and rows_of(V[rim]) <= rows_of(gotV)   # the boundary's vertices are where they were
    # with --flip-edges the collapse comes first, whatever the order given: the flips' line counts the collapsed mesh's edges
    # (a flip keeps their number) and ends with what a report of the written file finds
    both = reconstruct("both.ply", "--flip-edges", "64", "--collapse-edges", "0.3")
    assert len(both) == len(out) + 1 and both[:-2] == plain and re.fullmatch(pattern, both[-2])
    bothV, bothT = parse_ply_mesh(str(tmp_path / "both.ply"))
    flips = fc.flip(bothV, bothT, 0, 1e-6, 0.5)[1]
    collapsed = [int(x) for x in re.fullmatch(pattern, both[-2]).groups()[:12]]
    assert (len(bothV), len(bothT)) == (collapsed[9], collapsed[11]) and collapsed[:3] == [1, interior, fixed]
    assert re.match(r"flip-edges chunks 1 interior-edges %d rounds \d+ flips \d+ non-delaunay \d+ -> %d blocked %d "
                    % (flips["interiorEdges"], flips["nonDelaunayBefore"], flips["blockedAfter"]), both[-1]), both[-1]
    refused = subprocess.run([exe, "--weld", "host", "--collapse-edges", "0.3", str(tmp_path / "in.ply"), str(tmp_path / "host.ply"), "1.0",
                              "1.5", "4", "3", "0.02", "8000"], capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--collapse-edges needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
