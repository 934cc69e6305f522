"""The device long-edge split (mlsgpu_hip_mesh_split_edges, mlsgpu_hip_mesher_split_edges, reconstruct --split-edges) against
the CPU oracle of split_cases.py: every vertex bit, every triangle row, every pair of ends and every statistic.
test_split_oracle.py checks on the CPU that the inputs used here converge within MAX_ROUNDS."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import split_cases as sp
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_ROUNDS = 64
SINK_LENGTH = 0.6               # of the sink's grid spacing of 1
BIG_LENGTH = 1.35               # of the big grid's spacing of 1: the mesh roughly doubles (342 568 triangles in 6 rounds)
BAND = 0xABCD1234


def rows32(triangles):
    return (np.asarray(triangles, np.int64) & 0xFFFFFFFF).astype(np.uint32)


def run(ctx, vertices, triangles, max_length, max_rounds=MAX_ROUNDS, max_out_triangles=0, pinned=None):
    from mlsgpu_amd import binding as b
    return b.mesh_split_edges(ctx, vertices, rows32(triangles), max_rounds, max_length, max_out_triangles, pinned)


def check(ctx, vertices, triangles, max_length, max_rounds=MAX_ROUNDS, max_out_triangles=0, pinned=None):
    want = sp.split(vertices, triangles, max_rounds, max_length, max_out_triangles, pinned)
    sp.assert_same(run(ctx, vertices, triangles, max_length, max_rounds, max_out_triangles, pinned), want)
    return want


def small_meshes():
    return (sp.flat_grid(20, 20, 0.3, 1), sp.noisy_torus(40, 12, 0.004, 7), sp.fan_mesh(200, seed=1))


# ---------------------------------------------------------------- hand cases, small meshes, empty meshes

def test_hand_cases(ctx):
    v, t, st, ends = check(ctx, *sp.one_triangle(), 3.5)
    assert t.tolist() == [[0, 3, 2], [3, 1, 2]] and ends.tolist() == [[0, 1]] and v[3].tolist() == [2, 0, 0]
    assert (st["splits"], st["boundarySplits"], st["rounds"], st["converged"]) == (1, 1, 2, 1)
    v, t, st, ends = check(ctx, *sp.long_diagonal(), 2.5)
    assert t.tolist() == [[0, 4, 2], [4, 0, 3], [4, 1, 2], [1, 4, 3]] and ends.tolist() == [[0, 1]]
    st = check(ctx, *sp.fin(), 3.0)[2]
    assert (st["longBefore"], st["blockedAfter"], st["splits"], st["rounds"], st["converged"]) == (1, 1, 0, 1, 1)
    p, tri = sp.one_triangle()
    st = check(ctx, p, tri, 1.0, pinned=np.ones(3, np.uint8))[2]
    assert (st["blockedAfter"], st["longAfter"], st["rounds"], st["converged"], st["splits"]) == (3, 3, 1, 1, 0)
    for build in (sp.one_triangle, sp.long_diagonal, sp.tied_pair, sp.isosceles, sp.fin):
        for length in (0.3, 0.9, 1.7, 3.0):
            for rounds in (0, 1, 2, MAX_ROUNDS):
                check(ctx, *build(), length, rounds)
    p, tri = sp.defect_mesh()
    v, t, st, _ = check(ctx, p, tri, 0.7)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"]) == (2, 2) and st["splits"] > 20
    for row in (5, 77, 20, 121):                                    # the defect rows keep their bits and their place
        assert t[row].tolist() == rows32(tri)[row].tolist()


def test_small_meshes_at_three_lengths(ctx):
    for p, tri in small_meshes():
        longest = sp.longest_edge(p, tri)
        for factor in (0.7, 0.4, 0.2):
            st = check(ctx, p, tri, factor * longest)[2]
            assert st["converged"] == 1 and st["longAfter"] == 0 and st["splits"] > 0


def test_empty_meshes_and_pure_report(ctx):
    p, tri = sp.flat_grid(4, 4, 0.3, 1)
    v, t, st, ends = check(ctx, p, tri, 0.5, 0)                     # maxRounds = 0: a pure report, the output a copy
    assert v.tobytes() == p.tobytes() and t.tolist() == tri.tolist() and len(ends) == 0
    assert st["numEdges"] == 33 and st["longBefore"] == st["longAfter"] > 0 and st["qualityBefore"] == st["qualityAfter"]
    none = dict(sp.empty_stats(), rounds=1, converged=1)            # no triangle takes part: the first round finds no candidate
    assert check(ctx, p[:0], tri[:0], 0.5)[2] == none and check(ctx, p[:0], tri[:0], 0.5, 0)[2] == sp.empty_stats()
    v, t, st, _ = check(ctx, p, tri[:0], 0.5)                       # T = 0: the vertices come back
    assert v.tobytes() == p.tobytes() and len(t) == 0 and st == dict(none, numVertices=16, outVertices=16)
    assert check(ctx, p, tri[:0], 0.5, 0)[2]["rounds"] == 0
    v, t, st, _ = check(ctx, p[:0], tri, 0.5)                       # V = 0: every index is out of range, the rows keep their bits
    assert t.tolist() == tri.tolist() and st == dict(none, numTriangles=18, outOfRangeTriangles=18, outTriangles=18)


def test_classification_order(ctx):
    """An index >= V wins over a vertex twice, as for the flips; the rows stay where they are, and a row that names V does
    not come to life when a split makes a vertex V."""
    import topology_cases as tc
    p, tri = tc.classification_trap()
    _, t, st, _ = check(ctx, p, tri, 0.5)
    assert (st["outOfRangeTriangles"], st["degenerateTriangles"], st["numEdges"], st["interiorEdges"]) == (2, 1, 5, 1)
    assert st["outVertices"] > 8 and t[2:5].tolist() == tri[2:5].tolist()


# ---------------------------------------------------------------- several sort tiles, with growth

@pytest.fixture(scope="module")
def big_grid():
    p, tri = sp.grid_mesh(300, 300, jitter=0.3, seed=11)
    assert p.shape == (90_000, 3) and tri.shape == (178_802, 3)
    return p, tri, sp.split(p, tri, MAX_ROUNDS, BIG_LENGTH)


def test_several_sort_tiles_with_growth(ctx, big_grid):
    p, tri, want = big_grid
    st = want[2]
    print("big grid", dict((k, st[k]) for k in ("rounds", "splits", "outVertices", "outTriangles")))
    assert st["converged"] == 1 and st["rounds"] > 3 and st["splits"] > 50_000
    assert 1.5 * len(tri) < st["outTriangles"] < 3 * len(tri)       # the working arrays grow at least once
    sp.assert_same(run(ctx, p, tri, BIG_LENGTH), want)
    assert 3 * len(tri[:-1]) % 64 != 0 and len(tri[:-1]) % 64 != 0 and len(p) % 64 != 0       # a partial last wave
    check(ctx, p, tri[:-1], BIG_LENGTH)


# ---------------------------------------------------------------- one hub

def test_fan_around_one_hub(ctx):
    """One hub of valence 20 000: the reverse of every spoke is searched in a segment of 20 000 records, and every candidate
    of the first round touches the hub."""
    p, tri = sp.fan_mesh(20_000, seed=1)
    e = p[1:].astype(np.float64) - p[0].astype(np.float64)
    shortest_spoke = float(np.sqrt((e * e).sum(axis=1).min()))
    first = sp.split(p, tri, 1, 0.9 * shortest_spoke)
    assert first[2]["splits"] > 5_000 and (first[3][:, 0] == 0).all()       # the spokes longer than both their neighbours
    st = check(ctx, p, tri, 0.9 * shortest_spoke)[2]
    assert st["converged"] == 1 and st["longAfter"] == 0


# ---------------------------------------------------------------- closed surface, scaling

def test_closed_torus_and_scaling(ctx):
    from mlsgpu_amd import binding as b
    import topology_cases as tc
    p, tri = sp.noisy_torus(200, 40, 0.004, 7)
    length = 0.6 * sp.longest_edge(p, tri)
    v, t, st, ends = check(ctx, p, tri, length)
    assert st["converged"] == 1 and st["splits"] > 1000 and st["boundarySplits"] == 0 and st["numEdges"] == st["interiorEdges"] == 24_000
    keep = ("manifold", "numComponents", "numBoundaries", "boundaryEdges", "eulerCharacteristic")
    before, after = tc.report_fields(b.mesh_topology(ctx, rows32(tri), len(p))), tc.report_fields(b.mesh_topology(ctx, t, len(v)))
    assert before["manifold"] == 1 and [after[k] for k in keep] == [before[k] for k in keep]
    for shift in (-7, 40, -60):
        s = np.float32(2.0) ** np.float32(shift)
        got = run(ctx, p * s, tri, length * float(s))
        want = dict(st, maxLengthSqBefore=st["maxLengthSqBefore"] * float(s) ** 2, maxLengthSqAfter=st["maxLengthSqAfter"] * float(s) ** 2)
        sp.assert_same(got, (v * s, t, want, ends))


# ---------------------------------------------------------------- pins, the limit

def test_pinned_rim_and_limit(ctx):
    p, tri = sp.flat_grid(20, 20, 0.3, 1)
    length = 0.3 * sp.longest_edge(p, tri)
    st = check(ctx, p, tri, length, pinned=sp.rim_of(len(p), tri))[2]
    assert st["converged"] == 1 and st["longAfter"] > st["blockedAfter"] > 0
    sizes = [sp.split(p, tri, r, length)[2]["outTriangles"] for r in range(5)]
    assert sizes[2] < sizes[3] - 1
    v, t, st, ends = check(ctx, p, tri, length, max_out_triangles=sizes[3] - 1)
    assert (st["limited"], st["converged"], st["rounds"], st["outTriangles"]) == (1, 0, 2, sizes[2])
    sp.assert_same(run(ctx, p, tri, length, 2), (v, t, dict(st, limited=0), ends))
    st = check(ctx, p, tri, length, max_out_triangles=len(tri))[2]          # no room for the first round
    assert (st["limited"], st["rounds"], st["splits"], st["outTriangles"]) == (1, 0, 0, len(tri))
    assert check(ctx, p, tri, length, max_out_triangles=10 ** 9)[2]["limited"] == 0


# ---------------------------------------------------------------- counters, guard bands

def test_counters_guard_bands_and_size_query(ctx):
    from mlsgpu_amd import binding as b
    from mlsgpu_amd.split_stats import SplitStats
    p, tri = sp.defect_mesh()
    assert (tri == 0xFFFFFFFF).sum() == 1
    want = check(ctx, p, tri, 0.7)
    st = want[2]
    nv, nt, G = st["outVertices"], st["outTriangles"], 1024
    assert nv == len(p) + st["splits"] and nt == len(tri) + 2 * st["splits"] - st["boundarySplits"]
    rows = rows32(tri)
    dv, dt = b.DeviceBuffer(ctx, array=p), b.DeviceBuffer(ctx, array=rows)
    got = SplitStats()
    args = (ctx.h, dv.ptr, len(p), dt.ptr, len(tri), MAX_ROUNDS, 0.7, 0, None)
    entry = b.lib().mlsgpu_hip_mesh_split_edges
    with pytest.raises(b.LengthError, match="the result has %d and %d" % (nv, nt)):        # the size query: complete statistics
        b.check(entry(*args, None, 0, None, 0, None, C.byref(got)))
    assert got.as_dict() == st
    outs = [b.DeviceBuffer(ctx, array=np.full(2 * G + words, BAND, np.uint32)) for words in (3 * nv, 3 * nt, 2 * (nv - len(p)))]
    for cap_v, cap_t in ((nv - 1, nt), (nv, nt - 1)):               # one row short: nothing is written
        with pytest.raises(b.LengthError):
            b.check(entry(*args, outs[0].ptr + 4 * G, cap_v, outs[1].ptr + 4 * G, cap_t, outs[2].ptr + 4 * G, C.byref(got)))
        assert all((o.download(np.uint32) == BAND).all() for o in outs)
    b.check(entry(*args, outs[0].ptr + 4 * G, nv, outs[1].ptr + 4 * G, nt, outs[2].ptr + 4 * G, C.byref(got)))
    bands = [o.download(np.uint32) for o in outs]
    assert all((x[:G] == BAND).all() and (x[-G:] == BAND).all() for x in bands)
    sp.assert_same((bands[0][G:-G].view(np.float32), bands[1][G:-G], got.as_dict(), bands[2][G:-G]), want)
    assert dt.download(np.uint32).tobytes() == rows.tobytes()       # the inputs are left alone
    assert dv.download(np.float32).tobytes() == p.tobytes()
    for buf in [dv, dt] + outs:
        buf.free()


# ---------------------------------------------------------------- determinism

def test_determinism(ctx, big_grid):
    p, tri, want = big_grid
    a, b = run(ctx, p, tri, BIG_LENGTH), run(ctx, p, tri, BIG_LENGTH)
    assert all(x.tobytes() == y.tobytes() for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))) and a[2] == b[2]
    order = np.random.default_rng(3).permutation(len(tri))          # a permutation of the triangles: the same vertices and set
    got = run(ctx, p, tri[order], BIG_LENGTH)
    assert got[2] == want[2] and got[0].tobytes() == want[0].tobytes() and got[3].tolist() == want[3].tolist()
    assert sp.triangle_set(got[1]).tolist() == sp.triangle_set(want[1]).tolist()
    got = run(ctx, p, sp.rotated(tri, 4), BIG_LENGTH)               # rotated corners: the same again, q up to its last bit
    assert got[0].tobytes() == want[0].tobytes() and got[3].tolist() == want[3].tolist()
    assert sp.triangle_set(got[1]).tolist() == sp.triangle_set(want[1]).tolist()
    assert dict(got[2], **dict((k, want[2][k]) for k in sp.QUALITY_NAMES)) == want[2]


# ---------------------------------------------------------------- errors

def small_correct_call(ctx):
    check(ctx, *sp.flat_grid(9, 11, 0.45, 3), 0.8)


def test_errors_leave_the_context_usable(ctx):
    from mlsgpu_amd import binding as b
    from mlsgpu_amd.split_stats import SplitStats
    p, tri = sp.flat_grid(9, 11, 0.3, 3)
    p[40, 1] = np.nan
    p[60, 0] = np.inf
    with pytest.raises(sp.Invalid, match="vertex"):
        sp.split(p, tri, 2, 0.5)
    with pytest.raises(b.InvalidArgument, match="2 vertices have a coordinate that is not finite"):
        run(ctx, p, tri, 0.5, 2)
    with pytest.raises(b.InvalidArgument, match="2 vertices have a coordinate that is not finite"):
        run(ctx, p, tri[:0], 0.5, 2)
    small_correct_call(ctx)
    p, tri = sp.long_diagonal()
    for max_length, limit in [(0.0, 0), (-1.0, 0), (np.inf, 0), (np.nan, 0), (1.0, len(tri) - 1)]:
        with pytest.raises(sp.Invalid, match="parameters"):
            sp.split(p, tri, 1, max_length, limit)
        with pytest.raises(b.InvalidArgument):
            run(ctx, p, tri, max_length, 1, limit)
        small_correct_call(ctx)
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    entry = b.lib().mlsgpu_hip_mesh_split_edges
    with pytest.raises(b.InvalidArgument):
        b.check(entry(ctx.h, one.ptr, 1, one.ptr, 1, 1, 0.1, 0, None, one.ptr, 1, one.ptr, 1, None, None))
    st = SplitStats()
    for num_triangles, num_vertices in ((1, 2 ** 32), ((2 ** 32 + 2) // 3, 10)):
        with pytest.raises(b.LengthError):          # refused before anything is allocated or launched: the buffer holds 12 bytes
            b.check(entry(ctx.h, one.ptr, num_vertices, one.ptr, num_triangles, 1, 0.1, 0, None, one.ptr, 1, one.ptr, 1, None, C.byref(st)))
    one.free()
    small_correct_call(ctx)


# ---------------------------------------------------------------- the device sink

def file_bytes(path):
    with open(path, "rb") as f:
        return f.read()


def summed(stats):
    out = dict((name, sum(st[name] for st in stats)) for name in sp.STAT_NAMES if not name.startswith(("min", "max", "quality")))
    out["rounds"] = max(st["rounds"] for st in stats)
    out["converged"] = min(st["converged"] for st in stats)
    out["limited"] = max(st["limited"] for st in stats)
    for name in ("minQualityBefore", "minQualityAfter"):
        out[name] = min(st[name] for st in stats)
    for name in ("maxLengthSqBefore", "maxLengthSqAfter"):
        out[name] = max(st[name] for st in stats)
    for name in ("qualityBefore", "qualityAfter"):
        out[name] = [sum(st[name][k] for st in stats) for k in range(16)]
    return out


@pytest.mark.parametrize("chunks", [1, 2])
def test_sink(ctx, tmp_path, chunks):
    """One bucket in one chunk, eight buckets in two: each chunk is the oracle's for its own earlier download with the vertices
    the other chunk has too pinned, the seam's vertices and edges stay, the topology report's invariants stay, normals and
    files follow the new chunk, the limit holds per chunk, a finalize brings the chunks back."""
    import flip_cases as fc
    import normals_cases as nc
    import topology_cases as tc
    from mlsgpu_amd import binding as b
    from test_gpu_fill import in_rows
    from test_gpu_flip import seam_edges, summed as flips_summed
    from test_gpu_simplify import filled_sink
    from test_gpu_smooth import rows_of
    mesher, buckets = filled_sink(ctx, 47, lambda k: 0) if chunks == 1 else filled_sink(ctx, 24, lambda k: 7 if k < 4 else 3)
    with pytest.raises(b.InvalidArgument):
        mesher.split_edges(MAX_ROUNDS, SINK_LENGTH)                 # before finalize
    assert buckets == (1 if chunks == 1 else 8) and mesher.finalize() == chunks
    before = [mesher.chunk(i) for i in range(chunks)]
    keep = ("manifold", "numComponents", "numBoundaries", "eulerCharacteristic")
    topology = [tc.report_fields(mesher.chunk_topology(i)) for i in range(chunks)]
    shared = rows_of(before[0]["vertices"]) & rows_of(before[-1]["vertices"]) if chunks == 2 else set()
    seams = [seam_edges(c, shared) for c in before]
    assert chunks == 1 or (len(shared) > 100 and all(len(s) > 50 for s in seams))
    masks = [in_rows(c["vertices"], shared) if chunks == 2 else None for c in before]
    mesher.chunk_normals(0)                                         # computed before the call: must not be served after it
    want = [sp.split(c["vertices"], c["triangles"], MAX_ROUNDS, SINK_LENGTH, 0, m) for c, m in zip(before, masks)]
    st = mesher.split_edges(MAX_ROUNDS, SINK_LENGTH)
    print("sink", chunks, dict((k, st[k]) for k in ("splits", "boundarySplits", "rounds", "longBefore", "longAfter", "blockedAfter",
                                                    "outTriangles", "minQualityBefore", "minQualityAfter")))
    assert st == summed([w[2] for w in want]) and st["converged"] == 1 and st["splits"] > 1000
    assert (st["blockedAfter"] > 0) == (chunks == 2)                # the band along the seam
    for i in range(chunks):
        c = mesher.chunk(i)
        assert len(c["triangles"]) > len(before[i]["triangles"]) and c["chunk"] == before[i]["chunk"]
        sp.assert_same((c["vertices"], c["triangles"], want[i][2]), want[i])
        after = tc.report_fields(mesher.chunk_topology(i))
        assert [after[k] for k in keep] == [topology[i][k] for k in keep]
        assert after["boundaryEdges"] == topology[i]["boundaryEdges"] + want[i][2]["boundarySplits"]
        assert shared <= rows_of(c["vertices"]) and seam_edges(c, shared) == seams[i]      # the seam is as it was
        got = mesher.chunk_normals(i)
        nc.assert_same((got["normals"], got["stats"]), nc.normals(c["vertices"], want[i][1]))
        mesher.write_ply(i, tmp_path / "device.ply", comments=("c",))
        b.write_ply(tmp_path / "host.ply", want[i][0], want[i][1], comments=("c",))
        assert file_bytes(tmp_path / "device.ply") == file_bytes(tmp_path / "host.ply")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(b.InvalidArgument):
            mesher.split_edges(MAX_ROUNDS, bad)                     # a refused parameter costs no results
    again = mesher.split_edges(MAX_ROUNDS, SINK_LENGTH)             # it may be called again: a fixed point
    assert (again["splits"], again["rounds"], again["longBefore"], again["outTriangles"]) == (0, 1, st["longAfter"], st["outTriangles"])
    for i in range(chunks):
        assert mesher.chunk(i)["triangles"].tobytes() == want[i][1].tobytes()
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
    # a chunk's limit is maxGrowth times its triangles: at 1 no round has room
    limited = [sp.split(c["vertices"], c["triangles"], MAX_ROUNDS, SINK_LENGTH, len(c["triangles"]), m) for c, m in zip(before, masks)]
    st = mesher.split_edges(MAX_ROUNDS, SINK_LENGTH, max_growth=1)
    assert st == summed([w[2] for w in limited]) and (st["limited"], st["converged"], st["splits"]) == (1, 0, 0)
    mesher.close()


# ---------------------------------------------------------------- reconstruct --split-edges

def test_reconstruct_split_edges(ctx, tmp_path):
    """examples/reconstruct --split-edges 0.6: one more line, and a file that is a converged split of the file the same
    command writes without the option.  Two runs number their vertices in the order their worker threads deliver, and the
    vertex numbers break the ties between edges of equal length: the two files are compared through what does not depend on
    a tie (test_sink compares every bit, within one run).  The split comes before --flip-edges when both are given; refused
    for the host welder."""
    import flip_cases as fc
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

    pattern = (r"split-edges chunks (\d+) interior-edges (\d+) boundary-edges (\d+) rounds (\d+) splits (\d+) boundary (\d+) "
               r"long (\d+) -> (\d+) blocked (\d+) limited ([01]) vertices (\d+) -> (\d+) triangles (\d+) -> (\d+) "
               r"min-quality ([-+0-9.e]+) -> ([-+0-9.e]+) max-length ([-+0-9.e]+) -> ([-+0-9.e]+)")
    plain = reconstruct("plain.ply")
    out = reconstruct("out.ply", "--split-edges", str(SINK_LENGTH))
    assert len(out) == len(plain) + 1 and out[:-1] == plain, out
    V, tri = parse_ply_mesh(str(tmp_path / "plain.ply"))
    gotV, gotT = parse_ply_mesh(str(tmp_path / "out.ply"))
    st = sp.split(V, tri, 0, SINK_LENGTH)[2]                        # what the input's report says whatever the numbering
    line = re.fullmatch(pattern, out[-1])
    assert line, out[-1]
    (chunks, interior, boundary, rounds, splits, boundary_splits, long_before, long_after, blocked, limited, v_in, v_out, t_in,
     t_out) = [int(x) for x in line.groups()[:14]]
    assert (chunks, interior, boundary, long_before, v_in, t_in) == (1, st["interiorEdges"], st["boundaryEdges"], st["longBefore"], len(V), len(tri))
    assert float(line.group(15)) == float("%.9g" % st["minQualityBefore"])
    assert float(line.group(17)) == float("%.9g" % np.sqrt(st["maxLengthSqBefore"]))
    assert splits > 1000 and 1 < rounds <= 64 and (long_after, blocked, limited) == (0, 0, 0)
    assert (v_out, t_out) == (v_in + splits, t_in + 2 * splits - boundary_splits) == (len(gotV), len(gotT))
    assert float(line.group(18)) <= SINK_LENGTH
    again = sp.split(gotV, gotT, 64, SINK_LENGTH)[2]                # the file is a fixed point with the line's quality
    assert (again["splits"], again["longBefore"], again["rounds"]) == (0, 0, 1)
    assert float(line.group(16)) == float("%.9g" % again["minQualityBefore"])
    assert float(line.group(18)) == float("%.9g" % np.sqrt(again["maxLengthSqBefore"]))
    before, after = sp.invariants(len(V), tri), sp.invariants(len(gotV), gotT)
    assert after == dict(before, boundaryEdges=before["boundaryEdges"] + boundary_splits)
    assert rows_of(V) <= rows_of(gotV)                              # the input's vertices are where they were
    # with --flip-edges the split comes first, whatever the order given: the flips' line counts the split mesh's edges
    both = reconstruct("both.ply", "--flip-edges", "64", "--split-edges", str(SINK_LENGTH))
    assert len(both) == len(out) + 1 and both[:-2] == plain and re.fullmatch(pattern, both[-2])
    bothV, bothT = parse_ply_mesh(str(tmp_path / "both.ply"))
    flips = fc.flip(bothV, bothT, 0, 1e-6, 0.5)[1]
    split_line = [int(x) for x in re.fullmatch(pattern, both[-2]).groups()[:14]]
    assert (len(bothV), len(bothT)) == (split_line[11], split_line[13]) and split_line[:3] == [1, interior, boundary]
    assert re.match(r"flip-edges chunks 1 interior-edges %d rounds \d+ flips \d+ non-delaunay \d+ -> %d blocked %d "
                    % (flips["interiorEdges"], flips["nonDelaunayBefore"], flips["blockedAfter"]), both[-1]), both[-1]
    refused = subprocess.run([exe, "--weld", "host", "--split-edges", "0.6", str(tmp_path / "in.ply"), str(tmp_path / "host.ply"), "1.0",
                              "1.5", "4", "3", "0.02", "8000"], capture_output=True, timeout=300)
    assert refused.returncode != 0 and b"--split-edges needs --weld device" in refused.stderr
    assert not (tmp_path / "host.ply").exists()
