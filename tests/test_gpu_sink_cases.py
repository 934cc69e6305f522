"""The device mesh sink (csrc/mesher.hip) on the inputs of sink_cases.py: thousands of components (the general triangle
count of boundary(), both sides of its switch at 2 048 roots), several 4 096-element waves and sort tiles, 430 to 1 339 blocks
in interleaved chunks, keys shared by eight blocks in several chunks, empty blocks of every kind, long union-find chains at
three shortcut settings.  Everything is compared exactly: integers equal, meshes isomorphic (mesher_oracle.isomorphic),
the boundary export equal to mesher_oracle.expected_boundary element for element."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sink_cases as sc
from gpu_common import ctx  # noqa: F401
from sink_cases import CASES, STAT_NAMES, mo

pytestmark = pytest.mark.gpu

ALL = sorted(CASES)
_ORACLE, _FRESH = {}, {}


def oracle(name, prune):
    if (name, prune) not in _ORACLE:
        _ORACLE[name, prune] = mo.mesh_sink(CASES[name], prune)
    return _ORACLE[name, prune]


def fill(sink, meshes):
    """Adds the meshes; returns dense chunk number -> the case's chunk."""
    seen = {}
    for mesh in meshes:
        sink.add(seen.setdefault(mesh["chunk"], len(seen)), mesh["vertices"], mesh["num_internal"], mesh["keys"], mesh["triangles"])
    return {v: k for k, v in seen.items()}


def chunks_of(sink, n, back):
    out = [sink.chunk(i) for i in range(n)]
    return [(back[c["chunk"]], c["vertices"], c["triangles"]) for c in out]


def run_device(ctx, meshes, prune, background=False):  # noqa: F811
    import mlsgpu_amd as m
    sink = m.Mesher(ctx, prune)
    if background:
        sink.set_background(True)
    back = fill(sink, meshes)
    out = chunks_of(sink, sink.finalize(), back)
    stats = sink.stats()
    sink.close()
    return out, stats


def assert_matches_oracle(out, stats, exp, exp_stats):
    for k in STAT_NAMES:
        assert stats[k] == exp_stats[k], k
    assert [c for c, _, _ in out] == [c for c, _, _ in exp]                 # chunks in order of first arrival
    for (_, v, t), (_, ev, et) in zip(out, exp):
        assert mo.isomorphic(v, t, ev, et)


def assert_same_chunks(got, exp):
    assert [c for c, _, _ in got] == [c for c, _, _ in exp]
    for (_, v, t), (_, ev, et) in zip(got, exp):
        np.testing.assert_array_equal(v.view(np.uint32), ev.view(np.uint32))
        np.testing.assert_array_equal(t, et)


def assert_boundary_equal(got, exp):
    for g, e, what in zip(got, exp, ("keys", "key_root", "root_vertices", "root_triangles")):
        assert g.dtype == e.dtype and g.shape == e.shape, what
        np.testing.assert_array_equal(g, e, err_msg=what)


@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_finalize_matches_oracle(ctx, name, pruned):  # noqa: F811
    prune = sc.prune_of(name)[0] if pruned else 0.0
    exp, exp_stats = oracle(name, prune)
    if pruned and not name.startswith("ribbon_"):
        assert 0 < exp_stats["kept_components"] < exp_stats["components"]
    out, stats = run_device(ctx, CASES[name], prune, background=(ALL.index(name) + pruned) % 2 == 1)
    assert_matches_oracle(out, stats, exp, exp_stats)
    assert stats["vertices_added"] == sum(len(x["vertices"]) for x in CASES[name])
    assert stats["triangles_added"] == sum(len(x["triangles"]) for x in CASES[name])
    _FRESH[name, pruned] = (out, stats)


def fresh(ctx, name, pruned):  # noqa: F811
    """What a sink of its own makes of the case (kept from test_finalize_matches_oracle where that has run)."""
    if (name, pruned) not in _FRESH:
        _FRESH[name, pruned] = run_device(ctx, CASES[name], sc.prune_of(name)[0] if pruned else 0.0)
    return _FRESH[name, pruned]


@pytest.mark.parametrize("name", sc.TILED + ("empties",))
def test_boundary_equals_oracle(ctx, name):  # noqa: F811
    """boundary() exports exactly what the oracle predicts: keys ascending, a component's root its smallest welded vertex in
    (chunk by first arrival, arrival) order, roots numbered densely in that order.  The oracle's verdict through
    finalize_with() gives what finalize() gives at that threshold, and a boundary() behind a finalize() (which reuses its weld
    and components) exports the same arrays."""
    import mlsgpu_amd as m
    meshes = CASES[name]
    expected = sc.expected_boundary(name)
    prune, threshold = sc.prune_of(name)
    plain, plain_stats = fresh(ctx, name, True)
    sink = m.Mesher(ctx)
    back = fill(sink, meshes)
    assert_boundary_equal(sink.boundary(), expected)
    keep = (expected[2] >= threshold).astype(np.uint8)
    assert 0 < keep.sum() < len(keep)
    got = chunks_of(sink, sink.finalize_with(keep), back)
    assert_same_chunks(got, plain)
    stats = sink.stats()
    for k in ("total_vertices", "components", "kept_components", "kept_vertices", "kept_triangles"):
        assert stats[k] == plain_stats[k], k
    # the reuse path: finalize at the threshold, then the export
    sink.reset()
    sink.set_prune_threshold(prune)
    back = fill(sink, meshes)
    assert_same_chunks(chunks_of(sink, sink.finalize(), back), plain)
    assert_boundary_equal(sink.boundary(), expected)
    assert_same_chunks(chunks_of(sink, sink.finalize_with(keep), back), plain)
    sink.close()


@pytest.mark.parametrize("name,count", [("roots_2048", 2048), ("roots_2049", 2049)])
def test_boundary_on_either_side_of_the_component_switch(ctx, name, count):  # noqa: F811
    """2 048 roots take the per-workgroup bins, 2 049 the run-length kernel: both count every component's triangles."""
    import mlsgpu_amd as m
    sink = m.Mesher(ctx)
    fill(sink, CASES[name])
    got = sink.boundary()
    sink.close()
    assert len(got[2]) == len(got[3]) == count
    assert_boundary_equal(got, sc.expected_boundary(name))


def test_several_sinks_one_job(ctx):  # noqa: F811
    """test_gpu_mesher.test_several_device_sinks_one_job at a size where every sink has more than 2 048 components: blocks
    dealt round-robin to three sinks, every sink's export equal to the oracle's for its blocks, the merged statistics the
    single-sink oracle's, every sink's output the oracle's chunks for it."""
    import mlsgpu_amd as m
    from mlsgpu_amd import dist_sink
    meshes, ranks = CASES["many_components"], 3
    prune = sc.prune_of("many_components")[0]
    exp, exp_stats = mo.mesh_sink([dict(mm, chunk=(i % ranks, mm["chunk"])) for i, mm in enumerate(meshes)], prune)
    assert {k: exp_stats[k] for k in STAT_NAMES} == {k: oracle("many_components", prune)[1][k] for k in STAT_NAMES}
    sinks = [m.Mesher(ctx, prune) for _ in range(ranks)]
    backs = [fill(s, meshes[r::ranks]) for r, s in enumerate(sinks)]
    parts = [s.boundary() for s in sinks]
    for r, part in enumerate(parts):
        assert len(part[2]) > 2048
        assert_boundary_equal(part, mo.expected_boundary(meshes[r::ranks]))
    keep, stats = dist_sink.merge_boundaries(parts, prune)
    for k in STAT_NAMES:
        assert stats[k] == exp_stats[k], k
    kept_triangles = 0
    for r, s in enumerate(sinks):
        out = chunks_of(s, s.finalize_with(keep[r]), backs[r])
        mine = [(c[1], v, t) for c, v, t in exp if c[0] == r]
        assert [c for c, _, _ in out] == [c for c, _, _ in mine] and len(mine) > 1
        for (_, v, t), (_, ev, et) in zip(out, mine):
            assert mo.isomorphic(v, t, ev, et)
        kept_triangles += s.stats()["kept_triangles"]
        s.close()
    assert kept_triangles == exp_stats["kept_triangles"]


def test_one_sink_case_after_case(ctx):  # noqa: F811
    """One sink, reset() in between: block tables and chunk lists of very different lengths (247, 430, 115, 1 339 and 247
    blocks; 4, 5, 6, 7 and 4 chunks) behind one another.  Every result is what a sink of its own gives."""
    import mlsgpu_amd as m
    sink = m.Mesher(ctx)
    for name in ("corners", "many_components", "empties", "many_blocks", "corners"):
        exp, exp_stats = fresh(ctx, name, True)
        sink.set_prune_threshold(sc.prune_of(name)[0])
        back = fill(sink, CASES[name])
        got = chunks_of(sink, sink.finalize(), back)
        assert sink.stats() == exp_stats, name
        assert_same_chunks(got, exp)
        sink.reset()
    sink.close()


# ---- other union-find shortcuts and the peer route: read once per process, so each setting runs in a process of its own ----

def child_main():
    """In a fresh process (see test_shortcut_and_peer_route): the four ribbons and `corners` against the oracle, and under
    MLSGPU_HIP_MESHER_FORCE_PEER `empties` as well."""
    import mlsgpu_amd as m
    names = ["ribbon_" + n for n in sc.NUMBERINGS] + ["corners"]
    if os.environ.get("MLSGPU_HIP_MESHER_FORCE_PEER"):
        names.append("empties")
    context = m.Context(0)
    for name in names:
        for prune in (0.0, sc.prune_of(name)[0]):
            out, stats = run_device(context, CASES[name], prune)
            assert_matches_oracle(out, stats, *mo.mesh_sink(CASES[name], prune))
        print("ok", name, file=sys.stderr)
    context.close()


@pytest.mark.parametrize("shortcut,peer", [(0, True), (8, False)])
def test_shortcut_and_peer_route(shortcut, peer):
    """MLSGPU_HIP_UF_SHORTCUT = 0 (every walk re-parents its start) and 8 (the setting of meshes beyond 100 M vertices, out of
    a test's reach otherwise) on the ribbons, whose numberings make the longest chains, and on `corners`; the default runs
    in test_finalize_matches_oracle.  The first child also takes the peer route for every append (corners, empties)."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MLSGPU_HIP_UF_SHORTCUT=str(shortcut))
    env.pop("MLSGPU_HIP_MESHER_FORCE_PEER", None)
    if peer:
        env["MLSGPU_HIP_MESHER_FORCE_PEER"] = "1"
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_sink_cases as t; t.child_main()" % (tests, os.path.dirname(tests))
    done = subprocess.run([sys.executable, "-c", code], env=env, timeout=60, capture_output=True, text=True)
    if done.returncode != 0:
        print(done.stderr)
    assert done.returncode == 0, "child with shortcut %d failed" % shortcut
