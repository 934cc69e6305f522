"""The inputs of sink_cases.py have the properties the device sink's tests rely on (asserted from the inputs and the oracle
alone), the oracle's boundary export equals a brute-force one, and the HOST welder agrees with the oracle on every case:
statistics, chunks up to isomorphism, boundary up to its own clump numbering.  Host code: runs without a GPU."""
import numpy as np
import pytest

import sink_cases as sc
from mesher_cases import CASES as REFERENCE_CASES, random_meshes
from sink_cases import CASES, mo


def summary(meshes):
    L = mo.mesh_sink_labels(meshes)
    n = len(L["comp_rep"])
    return dict(blocks=len(meshes), added=n, welded=int((L["comp_rep"] == np.arange(n)).sum()), external=len(L["ext_key"]),
                triangles=len(L["triangles"]), components=len(np.unique(L["label"])))


def chunk_sequence(meshes):
    """Dense chunk index (first arrival) of every block, in arrival order."""
    seen = {}
    return np.array([seen.setdefault(m["chunk"], len(seen)) for m in meshes])


def blocks_per_key(meshes):
    """(distinct keys, number of blocks that hold each, block indices of every (key, block) pair sorted by key)."""
    keys = np.concatenate([m["keys"] for m in meshes])
    block = np.repeat(np.arange(len(meshes)), [len(m["keys"]) for m in meshes])
    for m in meshes:
        assert len(np.unique(m["keys"])) == len(m["keys"])              # a block holds a key once
    order = np.argsort(keys, kind="stable")
    distinct, count = np.unique(keys, return_counts=True)
    return distinct, count, np.split(block[order], np.cumsum(count)[:-1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_welded_vertices_have_unique_positions(name):
    meshes = CASES[name]
    L = mo.mesh_sink_labels(meshes)
    pos = np.concatenate([np.asarray(meshes[i]["vertices"], np.float32).reshape(-1, 3) for i in L["order"]])
    assert np.all(pos == np.round(pos)) and pos.min() >= 0 and pos.max() < (1 << 21)       # small integers
    reps = L["comp_rep"] == np.arange(len(pos))
    assert len(np.unique(pos[reps], axis=0)) == reps.sum()             # one position per welded vertex ...
    assert np.array_equal(pos, pos[L["comp_rep"]])                      # ... and every copy of it lies there
    for m in meshes:
        assert len(m["keys"]) == len(m["vertices"]) - m["num_internal"]
        assert len(m["triangles"]) == 0 or m["triangles"].max() < len(m["vertices"])


def test_many_components_properties():
    s = summary(CASES["many_components"])
    assert s["components"] > 2048                    # boundary()'s general triangle count
    assert s["welded"] > 3 * 4096                    # several waves of componentSizeKernel, with root changes inside them
    assert s["external"] > 3 * 4096                  # several tiles of the key sort
    assert s["triangles"] > 3 * 4096                 # several waves of componentTrianglesKernel
    assert s["blocks"] >= 300
    assert not np.all(np.diff(chunk_sequence(CASES["many_components"])) >= 0)      # interleaved: the sink regroups


@pytest.mark.parametrize("name,count", [("roots_2048", 2048), ("roots_2049", 2049)])
def test_roots_cases_sit_on_either_side_of_the_switch(name, count):
    assert summary(CASES[name])["components"] == count
    assert len(sc.expected_boundary(name)[2]) == count


def test_corners_properties():
    meshes = CASES["corners"]
    distinct, count, blocks = blocks_per_key(meshes)
    chunk = chunk_sequence(meshes)
    forced = sc.sheet_key(*np.array(sc.CORNERS).T)
    assert len(forced) >= 16
    assert np.all(count[np.searchsorted(distinct, forced)] == 8)        # every forced corner is in exactly eight blocks
    assert count.max() == 8 and (count == 8).sum() >= 16
    spread = one_chunk = 0
    for k in np.flatnonzero(count == 8):
        sequence = chunk[blocks[k]]                                     # chunks of the key's blocks, in arrival order
        if len(np.unique(sequence)) >= 3 and not np.all(np.diff(sequence) >= 0):
            spread += 1
        if len(np.unique(sequence)) == 1:
            one_chunk += 1
    assert spread >= 1 and one_chunk >= 1
    assert set(count) >= {1, 2, 3, 4, 8}                                # every shorter run of the weld's walks as well


def test_many_blocks_properties():
    meshes = CASES["many_blocks"]
    assert len(meshes) > 600                                            # more appends than the sink keeps pending (512)
    sequence = chunk_sequence(meshes)
    assert len(np.unique(sequence)) == 7 and not np.all(np.diff(sequence) >= 0)
    assert all(len(m["triangles"]) > 0 for m in meshes)


def test_empties_properties():
    meshes = CASES["empties"]
    kinds = [sc.block_kind(m) for m in meshes]
    regular = [i for i, k in enumerate(kinds) if k == "regular"]
    front, end = kinds[:regular[0]], kinds[regular[-1] + 1:]
    inner = [k for i, k in enumerate(kinds) if regular[0] < i < regular[-1]]
    for where in (front, inner, end):
        assert set(where) >= set(sc.EMPTY_KINDS)
    by_chunk = {}
    for m, k in zip(meshes, kinds):
        by_chunk.setdefault(m["chunk"], []).append(k)
    assert any(set(v) == {"no_vertices", "no_triangles"} for v in by_chunk.values())     # a chunk of blocks without triangles
    assert list(by_chunk.values())[-1] == ["no_vertices", "no_vertices"]                 # the last chunk starts past every vertex
    # keys of the blocks without triangles: some shared with other blocks, some nobody else has
    distinct, count, blocks = blocks_per_key(meshes)
    lonely = [k for k in range(len(distinct)) if count[k] == 1 and kinds[blocks[k][0]] == "no_triangles"]
    shared = [k for k in range(len(distinct)) if count[k] > 1 and any(kinds[b] == "no_triangles" for b in blocks[k])]
    assert lonely and shared
    fraction, threshold = sc.prune_of("empties")
    assert fraction == 0.01 and threshold > 3
    all_chunks, stats0 = mo.mesh_sink(meshes, 0.0)
    kept_chunks, stats = mo.mesh_sink(meshes, fraction)
    assert 0 < stats["kept_components"] < stats["components"]
    gone = {c for c, _, _ in all_chunks} - {c for c, _, _ in kept_chunks}
    assert len(gone) >= 1 and all(len(v) == 3 for c, v, _ in all_chunks if c in gone)    # the island's chunk disappears


@pytest.mark.parametrize("numbering", sc.NUMBERINGS)
def test_ribbon_properties(numbering):
    (m,) = CASES["ribbon_" + numbering]
    s = summary([m])
    assert s["components"] == 1 and s["welded"] == s["added"] == 2 * sc.RIBBON_COLUMNS
    # the numbering is what the name says, along the strip (column by column)
    along = np.lexsort((m["vertices"][:, 1], m["vertices"][:, 0]))     # vertex ids in strip order
    step = np.diff(along)
    assert {"ascending": np.all(step == 1), "descending": np.all(step == -1),
            "zigzag": np.all(np.sign(step) == np.resize([1, -1], len(step))) and np.all(np.abs(np.diff(step)) > 1),
            "shuffled": 0.3 < np.mean(step > 0) < 0.7}[numbering]


@pytest.mark.parametrize("name", sorted(CASES))
def test_prune_threshold_keeps_some_components(name):
    fraction, threshold = sc.prune_of(name)
    stats = mo.mesh_sink(CASES[name], fraction)[1]
    assert stats["threshold"] == threshold > 0
    if name.startswith("ribbon_"):
        assert stats["kept_components"] == stats["components"] == 1 and threshold == stats["total_vertices"]
    else:
        assert 0 < stats["kept_components"] < stats["components"]


# ---- the oracle's boundary export against plain loops ----

def brute_boundary(meshes):
    seen, chunks = {}, []
    for m in meshes:
        if m["chunk"] not in seen:
            seen[m["chunk"]] = len(chunks)
            chunks.append(m["chunk"])
    ordered = [m for c in chunks for m in meshes if m["chunk"] == c]    # chunk by first arrival, arrival within the chunk
    first_of_key, rep, tris, n = {}, [], [], 0
    for m in ordered:
        for j in range(len(m["vertices"])):
            g = n + j
            rep.append(g if j < m["num_internal"] else first_of_key.setdefault(int(m["keys"][j - m["num_internal"]]), g))
        tris += [[n + int(i) for i in t] for t in m["triangles"]]
        n += len(m["vertices"])
    comp = list(range(n))                                               # component = smallest representative, by relabelling
    changed = True
    while changed:
        changed = False
        for t in tris:
            low = min(comp[rep[i]] for i in t)
            for i in t:
                if comp[rep[i]] != low:
                    comp[rep[i]] = low
                    changed = True
    roots = sorted({comp[g] for g in range(n) if rep[g] == g})
    dense = {r: d for d, r in enumerate(roots)}
    rv, rt = [0] * len(roots), [0] * len(roots)
    for g in range(n):
        if rep[g] == g:
            rv[dense[comp[g]]] += 1
    for t in tris:
        rt[dense[comp[rep[t[0]]]]] += 1
    keys = sorted(first_of_key)
    return (np.array(keys, np.uint64), np.array([dense[comp[first_of_key[k]]] for k in keys], np.uint32),
            np.array(rv, np.uint64), np.array(rt, np.uint64))


@pytest.mark.parametrize("which", ["weld", "chunk", "random", "random_interleaved"])
def test_expected_boundary_equals_brute_force(which):
    meshes = {"weld": lambda: REFERENCE_CASES["weld"]["meshes"], "chunk": lambda: REFERENCE_CASES["chunk"]["meshes"][::-1],
              "random": lambda: random_meshes(1),
              "random_interleaved": lambda: [random_meshes(1)[i] for i in [0, 4, 8, 1, 5, 9, 2, 10, 6, 3, 7, 11]]}[which]()
    got, exp = mo.expected_boundary(meshes), brute_boundary(meshes)
    for g, e in zip(got, exp):
        assert g.dtype == e.dtype
        np.testing.assert_array_equal(g, e)


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_agree_with_mesh_sink(name):
    """mesh_sink welds with dictionaries in arrival order, mesh_sink_labels with sorts in grouped order: same statistics."""
    keys, key_root, rv, rt = sc.expected_boundary(name)
    stats = mo.mesh_sink(CASES[name])[1]
    assert stats["components"] == len(rv) and stats["total_vertices"] == rv.sum() and stats["kept_triangles"] == rt.sum()
    assert np.all(keys[1:] > keys[:-1]) and np.all(key_root < len(rv))


# ---- the host welder on every case ----

def run_host(meshes, prune):
    import mlsgpu_amd as m
    mesher = m.HostMesher(prune, threads=4)
    seen = {}
    for mesh in meshes:
        mesher.add(seen.setdefault(mesh["chunk"], len(seen)), mesh["vertices"], mesh["num_internal"], mesh["keys"], mesh["triangles"])
    n = mesher.finalize()
    out = [mesher.chunk(i) for i in range(n)]
    stats, boundary = mesher.stats(), mesher.boundary()
    mesher.close()
    back = {v: k for k, v in seen.items()}
    return [(back[c], v, t) for c, v, t in out], stats, boundary


def assert_boundary_up_to_numbering(got, exp):
    """got: a welder's (keys, key_clump, clump_vertices, clump_triangles) in a numbering of its own, clumps that are no roots
    zero; exp: the oracle's.  Same keys, same partition of the keys, same (vertices, triangles) per component."""
    keys, clump, cv, ct = got
    ekeys, root, rv, rt = exp
    np.testing.assert_array_equal(keys, ekeys)
    live = np.flatnonzero(cv > 0)
    assert sorted(zip(cv[live].tolist(), ct[live].tolist())) == sorted(zip(rv.tolist(), rt.tolist()))
    pairs = np.unique(np.stack([clump.astype(np.int64), root.astype(np.int64)], axis=1), axis=0)
    assert len(pairs) == len(np.unique(clump)) == len(np.unique(root))          # clump <-> root is one to one on the keys
    np.testing.assert_array_equal(cv[clump], rv[root])
    np.testing.assert_array_equal(ct[clump], rt[root])


@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_welder_matches_oracle(name, pruned):
    meshes = CASES[name]
    prune = sc.prune_of(name)[0] if pruned else 0.0
    exp, exp_stats = mo.mesh_sink(meshes, prune)
    out, stats, boundary = run_host(meshes, prune)
    for k in sc.STAT_NAMES:
        assert stats[k] == exp_stats[k], k
    assert [c for c, _, _ in out] == [c for c, _, _ in exp]
    for (_, v, t), (_, ev, et) in zip(out, exp):
        assert mo.isomorphic(v, t, ev, et)
    assert_boundary_up_to_numbering(boundary, sc.expected_boundary(name))
