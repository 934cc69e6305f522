"""A CPU oracle for the mesh repair (mlsgpu_hip_mesh_repair), and the meshes its tests share.

repair() follows the contract in include/mlsgpu_hip.h step by step: np.unique on the directed sides for the repeated ones, a
successor table over the corners (corner -> the corner of the triangle across its side out) closed by pointer doubling for
the umbrellas (no Python loop per vertex or per corner), np.minimum.at for the keys, np.unique on (vertex, key) for the
numbering.  Nothing here is product code.
"""
import numpy as np

import simplify_cases as sc
import topology_cases as tc
from fill_cases import soup  # noqa: F401  (the tests take it from here)
from simplify_cases import grid_mesh, torus_mesh  # noqa: F401
from smooth_cases import renumbered  # noqa: F401

SPLIT_PINCHES = 1
STAT_NAMES = ("numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "repeatedSides", "droppedTriangles",
              "unusedVertices", "splitVertices", "addedVertices", "outVertices", "outTriangles")


class Invalid(Exception):
    """What the device reports as MLSGPU_ERR_INVALID."""


def umbrellas(succ, longest):
    """For the table succ (corner -> the next corner of its umbrella, itself where the side out is open): an id per corner that
    the corners of one umbrella share, and whether the umbrella is a chain.  Pointer doubling: after k rounds a corner knows the
    smallest corner among the 2^k behind it and where 2^k steps lead; a chain's corners all arrive at its open end.  `longest`
    bounds an umbrella's corners."""
    n = len(succ)
    label = np.arange(n, dtype=np.int64)
    jump = succ.copy()
    for _ in range(int(longest).bit_length() + 1):
        label = np.minimum(label, label[jump])
        jump = jump[jump]
    chain = succ[jump] == jump
    return np.where(chain, jump, label), chain


def repair(vertices, triangles, flags=0):
    """(vertices float32 [V', 3], triangles uint32 [T', 3], statistics dict, source uint32 [V']) or Invalid."""
    if int(flags) & ~SPLIT_PINCHES:
        raise Invalid("flags")
    p = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    V, T = len(p), len(tri)
    stats = dict.fromkeys(STAT_NAMES, 0)
    stats.update(numVertices=V, numTriangles=T)

    # step 1
    bad = ((tri >= V) | (tri < 0)).any(axis=1)
    degenerate = ~bad & ((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0]))
    stats.update(outOfRangeTriangles=int(bad.sum()), degenerateTriangles=int(degenerate.sum()))
    live = ~bad & ~degenerate

    # step 2: the sides of the live triangles, corner 3 t + j leaves tri[t, j] for tri[t, j + 1]
    W = np.int64(V + 1)
    frm, to = tri, tri[:, [1, 2, 0]]
    code = np.where(live[:, None], frm * W + to, -1)
    _, inverse, uses = np.unique(code.ravel(), return_inverse=True, return_counts=True)
    repeated = (uses[inverse.reshape(-1)] > 1).reshape(T, 3) & live[:, None]
    stats["repeatedSides"] = int(repeated.sum())
    dropped = repeated.any(axis=1)
    stats["droppedTriangles"] = int(dropped.sum())
    kept = live & ~dropped
    kt = np.flatnonzero(kept)
    K = len(kt)
    stats["outTriangles"] = K
    if K == 0:
        stats["unusedVertices"] = V
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), stats, np.zeros(0, np.uint32)

    # step 3, over the corners of the kept triangles: local corner 3 k + j
    a, b = tri[kt].ravel(), tri[kt][:, [1, 2, 0]].ravel()          # corner c lies at a[c], its side out goes to b[c]
    order = np.argsort(a * W + b, kind="stable")
    sorted_code = (a * W + b)[order]
    assert (sorted_code[1:] != sorted_code[:-1]).all()              # the kept sides are unique
    want = b * W + a                                                # the opposite of every side
    at = np.minimum(np.searchsorted(sorted_code, want), 3 * K - 1)
    has = sorted_code[at] == want
    twin = order[at]                                                # the corner, at b, whose side out is b -> a
    nxt = twin - twin % 3 + (twin % 3 + 1) % 3                      # that triangle's next corner: it lies at a
    succ = np.where(has, nxt, np.arange(3 * K))
    assert (a[succ] == a).all()
    umbrella, chain = umbrellas(succ, np.bincount(a).max())

    # step 4
    heads = np.unique(umbrella)                                     # one corner per umbrella
    rings = np.bincount(a[heads], weights=(~chain[heads]).astype(np.float64), minlength=V).astype(np.int64)
    chains = np.bincount(a[heads], weights=chain[heads].astype(np.float64), minlength=V).astype(np.int64)
    # step 5: the smallest `to` of each umbrella, of each vertex's chains, of each vertex
    big = np.int64(V)
    least = np.full(3 * K, big)
    np.minimum.at(least, umbrella, b)
    least_chain = np.full(V, big)
    np.minimum.at(least_chain, a[chain], b[chain])
    least_all = np.full(V, big)
    np.minimum.at(least_all, a, b)
    if int(flags) & SPLIT_PINCHES:
        key = least[umbrella]
        groups = rings + chains
    else:
        mixed = (rings >= 1) & (rings + chains > 1)
        key = np.where(mixed[a], np.where(chain, least_chain[a], least[umbrella]), least_all[a])
        groups = np.where(mixed, rings + (chains > 0), (rings + chains > 0).astype(np.int64))
    group_code, index = np.unique(a * W + key, return_inverse=True)
    source = (group_code // W).astype(np.uint32)
    used = int((groups > 0).sum())
    stats.update(unusedVertices=V - used, splitVertices=int((groups > 1).sum()), addedVertices=len(group_code) - used,
                 outVertices=len(group_code))
    assert int(groups.sum()) == len(group_code)
    assert stats["outVertices"] == V - stats["unusedVertices"] + stats["addedVertices"]
    assert stats["outTriangles"] == T - stats["outOfRangeTriangles"] - stats["degenerateTriangles"] - stats["droppedTriangles"]
    # step 6
    return p[source], index.reshape(-1, 3).astype(np.uint32), stats, source


def assert_same(got, want):
    """(vertices, triangles, stats[, source]) against the oracle's: the positions as uint32 views, everything else exactly."""
    gv, gt, gs = got[:3]
    wv, wt, ws = want[:3]
    assert gs == ws, (gs, ws)
    gv = np.ascontiguousarray(gv, np.float32).reshape(-1, 3)
    assert gv.shape == wv.shape
    np.testing.assert_array_equal(gv.view(np.uint32), wv.view(np.uint32))
    np.testing.assert_array_equal(np.asarray(gt, np.uint32).reshape(-1, 3), wt)
    if len(got) > 3:
        np.testing.assert_array_equal(np.asarray(got[3], np.uint32), want[3])


def report(result):
    """topology_cases.count_all of a repair's output."""
    return tc.count_all(len(result[0]), result[1])


# ---------------------------------------------------------------- meshes

def positions(n, seed=0):
    """n distinct float32 positions."""
    p = np.random.default_rng(seed).random((n, 3)).astype(np.float32)
    p[:, 0] += np.arange(n, dtype=np.float32)
    return p


def bowtie(n=4, m=5, hub=0):
    """Two cones that share the vertex `hub` and nothing else: the hub TUNNELs between two rings.  The other vertices take the
    remaining numbers in order, the first cone's ring first."""
    others = np.array([i for i in range(n + m + 1) if i != hub], np.int64)
    a, b = tc.cone(n, 0, 1), tc.cone(m, 0, 1 + n)
    table = np.concatenate([[hub], others])
    return positions(n + m + 1, 1), table[np.concatenate([a, b])]


def fan(n, hub, first):
    """n triangles around `hub` over the n + 1 vertices first ..: an open fan, the hub on its boundary."""
    k = np.arange(n)
    return np.stack([np.full(n, hub), first + k, first + k + 1], axis=1).astype(np.int64)


def cone_and_fan(n=4, m=3):
    """A cone and an open fan on hub 0: the hub is MIXED."""
    return positions(1 + n + m + 1, 2), np.concatenate([tc.cone(n, 0, 1), fan(m, 0, 1 + n)])


def two_fans(n=2, m=3):
    """Two open fans on hub 0: a vertex on two boundary runs, which the reference allows."""
    return positions(1 + n + 1 + m + 1, 3), np.concatenate([fan(n, 0, 1), fan(m, 0, 2 + n)])


def fin(n=4, m=4):
    """A grid with a third triangle on one of its interior edges, in the direction of one of the two it has."""
    p, tri = grid_mesh(n, m)
    t = tri[2 * ((n - 1) * (m - 1) // 2)]
    extra = np.array([[t[0], t[1], len(p)]], np.int64)
    return np.concatenate([p, [[9.0, 9.0, 9.0]]]).astype(np.float32), np.concatenate([tri, extra])


def twice(n=3, m=4):
    """A grid one of whose triangles is given twice."""
    p, tri = grid_mesh(n, m)
    return p, np.concatenate([tri, tri[3:4]])


def simplified_torus(n, m, minor, cell):
    """torus_mesh(n, m, 0.5, minor) clustered at `cell` from origin (-1, -1, -1) by the simplify oracle."""
    p, tri = torus_mesh(n, m, 0.5, minor)
    v, t, _ = sc.simplify(p, tri, (-1.0, -1.0, -1.0), cell)
    return v, np.asarray(t, np.int64)


TORI = [(97, 61, 0.125, 0.03), (97, 61, 0.125, 0.06), (97, 61, 0.125, 0.11),
        (200, 90, 0.05, 0.03), (200, 90, 0.05, 0.06), (200, 90, 0.05, 0.11)]
