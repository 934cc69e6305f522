"""The device topology report (mlsgpu_hip_mesh_topology, mlsgpu_hip_mesher_chunk_topology) against closed forms, the
count-all CPU oracle of topology_cases.py and the restated Manifold::isManifold of refdata.py."""
import collections
import subprocess

import numpy as np
import pytest

import topology_cases as tc
from gpu_common import ctx  # noqa: F401
from refdata import is_manifold

pytestmark = pytest.mark.gpu

RANDOM_SEED = 2         # with it every verdict of is_manifold occurs at least 5 times among the 600 meshes (asserted below)


def report(ctx, num_vertices, triangles):
    from mlsgpu_amd import binding as b
    return tc.report_fields(b.mesh_topology(ctx, np.asarray(triangles).astype(np.uint32), num_vertices))


def assert_manifold(r, components, boundaries, euler=None):
    assert r["manifold"] == 1 and r["count"] == [0] * 6 and r["firstOf"] == [tc.U64_MAX] * 6, r
    assert (r["firstKind"], r["firstIndex"], r["duplicateEdges"]) == (tc.NONE, tc.U64_MAX, 0), r
    assert (r["numComponents"], r["numBoundaries"]) == (components, boundaries), r
    assert r["edges"] == (3 * r["numTriangles"] + r["boundaryEdges"]) // 2
    assert r["eulerCharacteristic"] == r["numVertices"] - r["edges"] + r["numTriangles"]
    if euler is not None:
        assert r["eulerCharacteristic"] == euler, r


# ---------------------------------------------------------------- closed forms

def test_torus(ctx):
    V, tri = tc.torus(4, 5)
    r = report(ctx, V, tri)
    assert_manifold(r, 1, 0, 0)
    assert r["boundaryEdges"] == 0 and r["edges"] == 3 * len(tri) // 2


@pytest.mark.parametrize("n,m", [(2, 2), (3, 7), (300, 300)])       # 300 x 300: 536 406 half-edges, several sort tiles
def test_open_grid(ctx, n, m):
    V, tri = tc.grid(n, m)
    r = report(ctx, V, tri)
    assert_manifold(r, 1, 1, 1)
    assert r["boundaryEdges"] == 2 * (n - 1) + 2 * (m - 1)


def test_five_grids(ctx):
    V, tri = tc.grid(3, 7)
    r = report(ctx, 5 * V, np.concatenate([tri + k * V for k in range(5)]))
    assert_manifold(r, 5, 5, 5)
    assert r["boundaryEdges"] == 5 * 16


def test_one_triangle(ctx):
    assert_manifold(report(ctx, 3, [[0, 1, 2]]), 1, 1, 1)


# ---------------------------------------------------------------- random family

def test_random_family(ctx):
    from mlsgpu_amd import binding as b
    rng = np.random.default_rng(RANDOM_SEED)
    cases = [tc.random_mesh(rng) for _ in range(600)]
    verdicts = [tc.verdict_of(is_manifold(V, tri)) for V, tri in cases]
    seen = collections.Counter(kind for kind, _ in verdicts)
    assert sorted(seen) == list(range(7)) and min(seen.values()) >= 5, seen
    for k, ((V, tri), (kind, index)) in enumerate(zip(cases, verdicts)):
        t = b.mesh_topology(ctx, tri.astype(np.uint32), V)
        r = tc.report_fields(t)
        assert r == tc.count_all(V, tri), k
        assert r["firstKind"] == kind, (k, r)
        if kind not in (tc.NONE, tc.DUPLICATED):
            assert r["firstIndex"] == index, (k, r)
        assert (b.reason(t) == "") == (kind == tc.NONE)


# ---------------------------------------------------------------- hubs

def test_hubs(ctx):
    n = 5000
    disc = tc.cone(n)
    assert_manifold(report(ctx, n + 1, disc), 1, 1, 1)
    r = report(ctx, n + 1, disc[1:])                        # the hub is on the boundary now
    assert_manifold(r, 1, 1, 1)
    assert r["boundaryEdges"] == n + 1
    two = np.concatenate([disc, tc.cone(n, 0, n + 1)])      # two discs that meet in the hub only
    r = report(ctx, 2 * n + 1, two)
    assert r["count"] == [0, 0, 0, 0, 0, 1] and r["firstOf"][tc.TUNNEL] == 0 and (r["firstKind"], r["firstIndex"]) == (tc.TUNNEL, 0)
    assert (r["manifold"], r["numComponents"], r["numBoundaries"], r["edges"], r["eulerCharacteristic"]) == (0, 0, 0, 0, 0)
    assert r["boundaryEdges"] == 2 * n
    extra = np.concatenate([disc, [[0, n + 1, n + 2]]])     # a closed fan and a loose triangle at the hub
    r = report(ctx, n + 3, extra)
    assert r["count"] == [0, 0, 0, 0, 1, 0] and (r["firstKind"], r["firstIndex"]) == (tc.MIXED, 0)
    assert r == tc.count_all(n + 3, extra)


# ---------------------------------------------------------------- untrusted indices

def test_untrusted_indices(ctx):
    V, tri = tc.grid(9, 11)
    bad = np.array([[0xFFFFFFFF, 1, 2], [3, V, 4], [5, 6, V + 1], [7, 7, 0xFFFFFFFF], [0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]], np.int64)
    at = [0, 17, 18, 90, len(tri) + 4]                     # positions of the bad triangles in the mixed list
    mixed = np.insert(tri, [0, 16, 16, 87, len(tri)], bad, axis=0)
    assert [mixed[i].tolist() for i in at] == bad.tolist()
    r = report(ctx, V, mixed)
    want = tc.count_all(V, mixed)
    assert r == want
    assert r["count"] == [4, 1, 0, 0, 0, 0] and r["firstOf"][:2] == [0, 90] and (r["firstKind"], r["firstIndex"]) == (tc.OUT_OF_RANGE, 0)
    good = report(ctx, V, tri)
    assert (r["boundaryEdges"], r["duplicateEdges"]) == (good["boundaryEdges"], 0)


def test_classification_order(ctx):
    """The hand case on which smoothing and hole filling classify differently (their tests have the other half)."""
    p, tri = tc.classification_trap()
    r = report(ctx, len(p), tri)
    tc.assert_trap_report(r)
    assert r == tc.count_all(len(p), tri)


# ---------------------------------------------------------------- edges of the API

def test_api_edges(ctx):
    from mlsgpu_amd import binding as b
    r = report(ctx, 3, np.zeros((0, 3), np.uint32))
    assert r["count"] == [0, 0, 3, 0, 0, 0] and (r["firstKind"], r["firstIndex"], r["manifold"]) == (tc.ISOLATED, 0, 0)
    assert r == tc.count_all(3, [])
    r = report(ctx, 0, np.zeros((0, 3), np.uint32))
    assert_manifold(r, 0, 0, 0)
    assert b.reason(b.mesh_topology(ctx, np.zeros((0, 3), np.uint32), 0)) == ""
    one = b.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    for num_triangles, num_vertices in (((2 ** 32 + 2) // 3, 10), (1, 2 ** 32)):
        with pytest.raises(b.LengthError):              # refused before any launch: the buffer holds one triangle
            b.mesh_topology(ctx, one, num_vertices, num_triangles)
    assert b.lib().mlsgpu_hip_mesh_topology(ctx.h, one.ptr, 1, 3, None) == 1
    with pytest.raises(b.InvalidArgument):
        b.check(b.lib().mlsgpu_hip_mesh_topology(ctx.h, None, 1, 3, None))
    with pytest.raises(b.InvalidArgument):
        b.mesh_topology(ctx, b.DeviceBuffer(ctx, borrow=0, nbytes=0), 3, 1)      # triangles claimed, none given
    one.free()


# ---------------------------------------------------------------- the sink's real output

SPLATS, EXTENT = 20_000, 47.0


def shells():
    from mlsgpu_amd import synth
    return synth.shells_cloud(SPLATS, EXTENT, 16.0, 1.5, 2.5, seed=5)       # grid units


def test_sink_output(ctx):
    """Eight buckets of a shells cloud through a worker into the device sink: the welded, pruned chunk is manifold where it
    lies, the downloaded chunk says the same under the CPU oracle, and one flipped face is found."""
    import mlsgpu_amd as m
    from mlsgpu_amd import binding as b, synth
    allb, buckets = synth.bucketize(shells(), int(EXTENT) + 1, 24)
    assert len(buckets) == 8
    dev = m.DeviceBuffer(ctx, array=allb)
    worker = m.Worker(ctx, max(bk.count for bk in buckets), max_cells=63)
    mesher = m.Mesher(ctx, 0.02)
    for bk in buckets:
        worker.process(dev, bk.first, bk.count, bk.low, bk.num_vertices, collector=mesher.collector(ctx, 0))
    assert mesher.finalize() == 1
    t = mesher.chunk_topology(0)
    r = tc.report_fields(t)
    got = mesher.chunk(0)
    V, tri = got["num_vertices"], got["triangles"]
    assert len(tri) > 1000 and mesher.stats()["total_vertices"] < mesher.stats()["vertices_added"]     # welded across buckets
    want = tc.count_all(V, tri)
    assert b.reason(t) == "" and r["manifold"] == 1, (b.reason(t), r)
    assert r == want
    assert (r["numVertices"], r["numTriangles"], r["numComponents"] >= 1) == (V, len(tri), True)
    with pytest.raises(b.InvalidArgument):
        mesher.chunk_topology(1)
    # the same triangles in a buffer of their own, one face flipped there
    flipped = tri.copy()
    k = len(tri) // 2
    flipped[k] = flipped[k][[0, 2, 1]]
    buf = b.DeviceBuffer(ctx, nbytes=tri.nbytes)
    buf.copy_from(b.DeviceBuffer(ctx, borrow=got["d_triangles"], nbytes=tri.nbytes))
    buf.upload(flipped[k], offset=12 * k)
    r = tc.report_fields(b.mesh_topology(ctx, buf, V))
    want = tc.count_all(V, flipped)
    assert r == want
    assert r["firstKind"] == tc.DUPLICATED and r["duplicateEdges"] == 3 and r["manifold"] == 0
    assert tc.verdict_of(is_manifold(V, flipped))[0] == tc.DUPLICATED
    buf.free()
    mesher.close()
    del worker
    dev.free()


def test_reconstruct_check(ctx, tmp_path):
    """examples/reconstruct --check --weld device: one more line per output chunk, whose numbers are the CPU oracle's for
    the file it wrote."""
    from test_host_cpp import build_example, parse_ply_mesh
    from mlsgpu_amd import synth
    exe = build_example(tmp_path, "reconstruct")
    cloud = shells()
    rows = np.zeros(len(cloud), synth.PLY_ROW)
    rows["p"], rows["n"], rows["r"] = cloud["position"], cloud["normal"], cloud["radius"]
    (tmp_path / "in.ply").write_bytes(synth.ply_header(len(rows)) + rows.tobytes())
    args = [str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "1.0", "1.5", "4", "3", "0.02", "8000"]
    out = subprocess.check_output([exe, "--weld", "device", "--check"] + args, timeout=300).decode().splitlines()
    assert len(out) == 2 and out[0].startswith("files in 1") and "weld device" in out[0], out
    V, tri = parse_ply_mesh(str(tmp_path / "out.ply"))
    want = tc.count_all(len(V), tri)
    assert want["manifold"] == 1 and len(tri) > 1000
    assert out[1] == "topology chunk 0 manifold yes components %d boundaries %d euler %d boundary-edges %d" % (
        want["numComponents"], want["numBoundaries"], want["eulerCharacteristic"], want["boundaryEdges"])
    out = subprocess.check_output([exe, "--weld", "host", "--check"] + args, timeout=300).decode().splitlines()
    assert len(out) == 1 and out[0].startswith("files in 1"), out           # device weld only
