"""The three routes a stage takes over the chunks of the device sink (mesher.hip: in place, into a new generation, to the
front), on hand meshes: a chain across all of them, a failure in the middle of a walk, a refused parameter.  The per-stage
test_sink cases compare a sink's chunks with the numpy oracles; here every chunk is compared, bit for bit, with what the
matching mesh_* call makes of the chunk's earlier download, and the sink's statistics with the fold of theirs."""
import numpy as np
import pytest

import collapse_cases as cc
import fill_cases as fl
import flip_cases as fc
import repair_cases as rc
import simplify_quadric_cases as sq
import smooth_cases as sc
from gpu_common import ctx  # noqa: F401

MAX_EDGES = 16                  # the grid's punched hole has 12 sides, its rim 44
ORIGIN, CELL = (-2.0, -2.0, -2.0), 0.1          # clusters the torus only: the other two chunks have no scale
ITERATIONS, LAMBDA, MU = 2, 0.5, -0.53
MAX_ROUNDS = 64
MAX_LENGTH = 0.1
# dense chunks without triangles (blocks without vertices) lie before and between the three that have some
CHUNK_IDS = (0, 1, 2, 3, 5)


def rows32(triangles):
    return np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)


def hand_meshes():
    """[(vertices, triangles)] of the chunks 0, 2 and 5: closed and tiny; open, with a hole and four unused vertices; closed."""
    return [sc.octahedron(), fl.punched(12, 12, [(4, 4, 3, 3)], jitter=0.3, seed=4), sc.noisy_torus(40, 12, 0.01, 1)]


def build_sink(ctx, meshes):  # noqa: F811
    """A sink with the meshes as the chunks 0, 2 and 5: all vertices internal, no keys, nothing pruned."""
    from mlsgpu_amd import binding as b
    mesher = b.Mesher(ctx)
    meshes = list(meshes)
    none = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    for chunk_id in CHUNK_IDS:
        v, t = none if chunk_id in (1, 3) else meshes.pop(0)
        mesher.add(chunk_id, v, len(v), np.zeros(0, np.uint64), rows32(t))
    return mesher


def stages(b):
    """(name, the sink's call, the mesh_* call on one chunk -> (vertices, triangles, statistics)), in the chain's order."""
    return [
        ("repair", lambda m: m.repair(0), lambda ctx, v, t: b.mesh_repair(ctx, v, t, 0)),
        ("fill_holes", lambda m: m.fill_holes(MAX_EDGES), lambda ctx, v, t: b.mesh_fill_holes(ctx, v, t, MAX_EDGES)),
        ("simplify_quadric", lambda m: m.simplify_quadric(ORIGIN, CELL), lambda ctx, v, t: b.mesh_simplify_quadric(ctx, v, t, ORIGIN, CELL)),
        ("smooth", lambda m: m.smooth(ITERATIONS, LAMBDA, MU), lambda ctx, v, t: insert(1, t, b.mesh_smooth(ctx, v, t, ITERATIONS, LAMBDA, MU))),
        ("flip_edges", lambda m: m.flip_edges(MAX_ROUNDS), lambda ctx, v, t: insert(0, v, b.mesh_flip_edges(ctx, v, t, MAX_ROUNDS))),
        ("collapse_edges", lambda m: m.collapse_edges(MAX_ROUNDS, MAX_LENGTH), lambda ctx, v, t: b.mesh_collapse_edges(ctx, v, t, MAX_ROUNDS, MAX_LENGTH)),
    ]


def insert(at, array, result):
    """(output, statistics) of a stage that changes one array, with the other one where it belongs."""
    return (result[0], array, result[1]) if at == 1 else (array, result[0], result[1])


# how a statistic of the sink follows from the chunks'; every other one is their sum (a histogram's element by element)
FOLD = dict(rounds="max", converged="and", passes="last", longestLoop="max", scaleExponent="max", maxMove="max", maxCoordinate="max",
            minQualityBefore="min", minQualityAfter="min", minLengthSqBefore="min", minLengthSqAfter="min")


def folded(stage, stats):
    """The sink's statistics from those of its chunks with triangles, in their order."""
    out = {}
    for name in stats[0]:
        values = [st[name] for st in stats]
        if stage == "simplify_quadric" and name == "scaleExponent":     # of the chunks that have a scale: where M != 0
            values = [st[name] for st in stats if st["solvedVertices"] + st["escapedVertices"] > 0] or [0]
        rule = FOLD.get(name, "sum")
        if isinstance(values[0], list):
            assert rule == "sum"
            out[name] = [sum(column) for column in zip(*values)]
        else:
            out[name] = {"sum": sum, "max": max, "min": min, "and": lambda x: int(all(x)), "last": lambda x: x[-1]}[rule](values)
    return out


def test_fold_table():
    """The table against the folds the per-stage tests have used since each stage came, on made-up chunks."""
    from test_gpu_collapse import summed as collapse_summed
    from test_gpu_smooth import summed as smooth_summed
    rng = np.random.default_rng(1)
    chunks = [dict((name, [int(x) for x in rng.integers(0, 9, 16)] if name.startswith("quality") else float(rng.random())
                    if name.startswith("min") else int(rng.integers(0, 9))) for name in cc.STAT_NAMES) for _ in range(3)]
    for st, converged in zip(chunks, (1, 0, 1)):
        st["converged"] = converged
    assert folded("collapse_edges", chunks) == collapse_summed(chunks) and folded("collapse_edges", chunks[::2])["converged"] == 1
    chunks = [dict((name, int(rng.integers(-9, 9))) for name in sc.STAT_NAMES) for _ in range(3)]
    for st in chunks:
        st["passes"] = 4
    assert folded("smooth", chunks) == smooth_summed(chunks)
    chunks = [dict.fromkeys(sq.STAT_NAMES, 0) for _ in range(3)]
    chunks[0].update(scaleExponent=13)
    chunks[1].update(scaleExponent=-3, solvedVertices=1)
    chunks[2].update(scaleExponent=-5, escapedVertices=2)
    assert folded("simplify_quadric", chunks)["scaleExponent"] == -3 and folded("fill_holes", chunks)["scaleExponent"] == 13


def test_oracles_accept_the_inputs():
    """On the CPU: the numpy oracles take the hand meshes through the chain, no two chunks share a position (no seam is
    pinned), and every stage changes something on at least one chunk."""
    meshes = hand_meshes()
    rows = [set(map(bytes, np.ascontiguousarray(p, np.float32).view("V12").ravel())) for p, _ in meshes]
    assert not (rows[0] & rows[1] or rows[0] & rows[2] or rows[1] & rows[2])
    changed = dict.fromkeys(("unusedVertices", "filledLoops", "collapsedTriangles", "maxMove", "flips", "collapses"), 0)
    scaled = []
    for p, t in meshes:
        v, t, st = rc.repair(p, t, 0)[:3]
        changed["unusedVertices"] += st["unusedVertices"]
        v, t, st = fl.fill(v, t, MAX_EDGES)
        changed["filledLoops"] += st["filledLoops"]
        v, t, st = sq.simplify_quadric(v, t, ORIGIN, CELL)[:3]
        changed["collapsedTriangles"] += st["collapsedTriangles"]
        scaled.append(st["solvedVertices"] + st["escapedVertices"] > 0)
        v, st = sc.smooth(v, t, ITERATIONS, LAMBDA, MU)
        changed["maxMove"] += st["maxMove"]
        t, st = fc.flip(v, t, MAX_ROUNDS)
        changed["flips"] += st["flips"]
        assert st["converged"] == 1
        st = cc.collapse(v, t, MAX_ROUNDS, MAX_LENGTH)[2]
        changed["collapses"] += st["collapses"]
        assert st["converged"] == 1 and st["outTriangles"] > 0
    assert all(x > 0 for x in changed.values()), changed
    assert scaled == [False, False, True]           # the sink's scaleExponent is the torus's, not the largest of the three
    p, t = meshes[2]                                # what test 2 relies on
    with pytest.raises(sc.Invalid, match="diverged"):
        sc.smooth(p, t, 80, 0.3, -1.0)


def downloads(mesher, count):
    return [mesher.chunk(i) for i in range(count)]


def same_bytes(chunks, want):
    return len(chunks) == len(want) and all(c["chunk"] == w["chunk"] and c["vertices"].tobytes() == w["vertices"].tobytes()
                                            and c["triangles"].tobytes() == w["triangles"].tobytes() for c, w in zip(chunks, want))


@pytest.mark.gpu
def test_chain_across_the_routes(ctx):  # noqa: F811
    """repair -> fill_holes -> simplify_quadric -> smooth -> flip_edges -> collapse_edges: new generation twice, to the front,
    in place twice, new generation."""
    from mlsgpu_amd import binding as b
    mesher = build_sink(ctx, hand_meshes())
    assert mesher.finalize() == 3
    before = downloads(mesher, 3)
    assert [c["chunk"] for c in before] == [0, 2, 5] and [len(c["triangles"]) for c in before] == [8, 224, 960]
    now = before
    for name, on_sink, on_mesh in stages(b):
        stale = [mesher.chunk_normals(i)["normals"] for i in range(3)]     # computed before the step: must not be served after it
        want = [on_mesh(ctx, c["vertices"], c["triangles"]) for c in now]
        got = on_sink(mesher)
        assert got == folded(name, [w[2] for w in want]), name
        now = downloads(mesher, 3)
        for i, (c, w) in enumerate(zip(now, want)):
            assert c["chunk"] == before[i]["chunk"], name
            assert c["vertices"].tobytes() == w[0].tobytes() and c["triangles"].tobytes() == w[1].tobytes(), (name, i)
            normals, st = b.mesh_normals(ctx, w[0], w[1])
            served = mesher.chunk_normals(i)
            assert served["normals"].tobytes() == normals.tobytes() and served["stats"] == st, (name, i)
        assert any(s.tobytes() != mesher.chunk_normals(i)["normals"].tobytes() for i, s in enumerate(stale)), name
        print(name, dict((k, got[k]) for k in list(got)[:2]))
    assert [len(c["triangles"]) for c in now][:2] == [8, 236] and 0 < len(now[2]["triangles"]) < 586
    assert mesher.finalize() == 3 and same_bytes(downloads(mesher, 3), before)
    mesher.close()


@pytest.mark.gpu
def test_failure_on_the_last_chunk(ctx):  # noqa: F811
    """One coordinate of the last chunk is not finite, which every stage that reads positions refuses on the host.  Into a new
    generation, nothing of the sink has changed by then; in place, the chunks before are smoothed already, so the results go."""
    import topology_cases as tc
    from mlsgpu_amd import binding as b
    meshes = hand_meshes()
    meshes[2][0][100, 1] = np.nan
    mesher = build_sink(ctx, meshes)
    assert mesher.finalize() == 3
    before = downloads(mesher, 3)
    assert before[2]["vertices"].tobytes() == meshes[2][0].tobytes()        # the sink neither refuses nor alters the vertex
    topology = [tc.report_fields(mesher.chunk_topology(i)) for i in range(3)]
    for call in (lambda: mesher.fill_holes(MAX_EDGES), lambda: mesher.collapse_edges(MAX_ROUNDS, MAX_LENGTH)):
        with pytest.raises(b.InvalidArgument, match="not finite"):
            call()
        assert same_bytes(downloads(mesher, 3), before)
        assert [tc.report_fields(mesher.chunk_topology(i)) for i in range(3)] == topology
    with pytest.raises(b.InvalidArgument, match="not finite"):
        mesher.smooth(ITERATIONS, LAMBDA, MU)
    for call in (lambda: mesher.chunk(0), lambda: mesher.chunk_topology(0), lambda: mesher.smooth(ITERATIONS, LAMBDA, MU)):
        with pytest.raises(b.InvalidArgument):
            call()
    assert mesher.finalize() == 3 and same_bytes(downloads(mesher, 3), before)
    want = [b.mesh_repair(ctx, c["vertices"], c["triangles"], 0) for c in before]      # the sink is usable: repair reads no position
    assert mesher.repair(0) == folded("repair", [w[2] for w in want])
    assert all(c["vertices"].tobytes() == w[0].tobytes() and c["triangles"].tobytes() == w[1].tobytes()
               for c, w in zip(downloads(mesher, 3), want))
    mesher.close()


@pytest.mark.gpu
def test_a_refused_parameter_costs_nothing(ctx):  # noqa: F811
    from mlsgpu_amd import binding as b
    refused = [lambda m: m.repair(2), lambda m: m.fill_holes(2), lambda m: m.simplify_quadric(ORIGIN, 0.0),
               lambda m: m.smooth(ITERATIONS, 0.0, MU), lambda m: m.flip_edges(MAX_ROUNDS, min_cos=2.0),
               lambda m: m.collapse_edges(MAX_ROUNDS, MAX_LENGTH, min_cos=2.0)]
    mesher = build_sink(ctx, hand_meshes())
    for call in refused:
        with pytest.raises(b.InvalidArgument):
            call(mesher)                            # before finalize
    assert mesher.finalize() == 3
    before = downloads(mesher, 3)
    for call in refused:
        with pytest.raises(b.InvalidArgument):
            call(mesher)
        assert same_bytes(downloads(mesher, 3), before)
    got = mesher.flip_edges(MAX_ROUNDS)             # and the sink works on
    assert got["flips"] > 0 and got["numTriangles"] == 8 + 224 + 960
    mesher.close()
