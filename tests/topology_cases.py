"""Meshes and a CPU oracle for the topology report (mlsgpu_hip_mesh_topology).

count_all() is the "count-all" form of Manifold::isManifold (test/manifold.h:98-232), written from its definition in
include/mlsgpu_hip.h: every triangle and vertex is classified and counted instead of returning at the first defect.
Nothing here is product code.
"""
import re

import numpy as np

OUT_OF_RANGE, DEGENERATE, ISOLATED, DUPLICATED, MIXED, TUNNEL, NONE = range(7)
U64_MAX = 2 ** 64 - 1


class _Forest:
    def __init__(self, n):
        self.parent = list(range(n))
        self.size = [1] * n

    def find(self, a):
        p = self.parent
        while p[a] != a:
            p[a] = p[p[a]]
            a = p[a]
        return a

    def merge(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            if self.size[a] < self.size[b]:
                a, b = b, a
            self.parent[b] = a
            self.size[a] += self.size[b]

    def roots(self, min_size=1):
        return sum(1 for i, p in enumerate(self.parent) if p == i and self.size[i] >= min_size)


def count_all(num_vertices, triangles):
    """The report as a dict with the fields of mlsgpu_topology (count and firstOf as lists)."""
    V = int(num_vertices)
    tri = np.asarray(triangles, np.int64).reshape(-1, 3)
    T = len(tri)
    count = [0] * 6
    first = [U64_MAX] * 6
    i0, i1, i2 = tri[:, 0], tri[:, 1], tri[:, 2]
    checks = np.stack([i0 >= V, i0 == i1, i1 >= V, i1 == i2, i2 >= V, i2 == i0], axis=1)
    bad = checks.any(axis=1)
    kind = np.where(np.argmax(checks, axis=1) % 2 == 0, OUT_OF_RANGE, DEGENERATE)
    for k in (OUT_OF_RANGE, DEGENERATE):
        which = np.nonzero(bad & (kind == k))[0]
        count[k] = len(which)
        if len(which):
            first[k] = int(which[0])
    good = tri[~bad]
    frm = np.concatenate([good[:, 0], good[:, 1], good[:, 2]])
    to = np.concatenate([good[:, 1], good[:, 2], good[:, 0]])
    third = np.concatenate([good[:, 2], good[:, 0], good[:, 1]])
    order = np.lexsort((to, frm))
    frm, to, third = frm[order], to[order], third[order]
    repeat = np.zeros(len(frm), bool)
    repeat[1:] = (frm[1:] == frm[:-1]) & (to[1:] == to[:-1])
    code = frm * (V + 1) + to
    distinct = ~repeat
    has_twin = np.isin(to * (V + 1) + frm, code)
    boundary = distinct & ~has_twin
    used = np.zeros(V, bool)
    used[good.ravel()] = True
    duplicated = np.zeros(V, bool)
    duplicated[frm[repeat]] = True
    duplicated[to[repeat]] = True
    seg = np.searchsorted(frm, np.arange(V + 1))
    vertex_class = np.full(V, NONE)
    for v in range(V):
        if not used[v]:
            vertex_class[v] = ISOLATED
            continue
        if duplicated[v]:
            vertex_class[v] = DUPLICATED
            continue
        xs = [int(x) for x in to[seg[v]:seg[v + 1]]]
        ys = [int(y) for y in third[seg[v]:seg[v + 1]]]
        arrow = dict(zip(xs, ys))
        seen = set(ys)
        assert len(arrow) == len(xs) and len(seen) == len(ys)
        length = 0
        starts = [x for x in xs if x not in seen]
        for x in starts:
            cur = x
            while cur in arrow:
                cur = arrow[cur]
                length += 1
        if starts:
            if length != len(xs):
                vertex_class[v] = MIXED
        else:
            cur = xs[0]
            while True:
                cur = arrow[cur]
                length += 1
                if cur == xs[0]:
                    break
            if length != len(xs):
                vertex_class[v] = TUNNEL
    for k in (ISOLATED, DUPLICATED, MIXED, TUNNEL):
        which = np.nonzero(vertex_class == k)[0]
        count[k] = len(which)
        if len(which):
            first[k] = int(which[0])
    out = dict(numVertices=V, numTriangles=T, count=count, firstOf=first, duplicateEdges=int(repeat.sum()),
               boundaryEdges=int(boundary.sum()), edges=0, numComponents=0, numBoundaries=0, eulerCharacteristic=0,
               firstIndex=U64_MAX, firstKind=NONE, manifold=int(not any(count)))
    for group in ((OUT_OF_RANGE, DEGENERATE), (ISOLATED, DUPLICATED, MIXED, TUNNEL)):
        for k in group:
            if first[k] < out["firstIndex"]:
                out["firstIndex"], out["firstKind"] = first[k], k
        if out["firstKind"] != NONE:
            break
    if out["manifold"]:
        out["edges"] = (3 * T + out["boundaryEdges"]) // 2
        out["eulerCharacteristic"] = V - out["edges"] + T
        comps = _Forest(V)
        for a, b in zip(frm[distinct].tolist(), to[distinct].tolist()):
            comps.merge(a, b)
        out["numComponents"] = comps.roots()
        # the reference's second union-find, test/manifold.h:193-195,223-227: sets of at least three vertices
        loops = _Forest(V)
        for a, b in zip(frm[boundary].tolist(), to[boundary].tolist()):
            loops.merge(a, b)
        out["numBoundaries"] = loops.roots(3)
    return out


def report_fields(t):
    """A binding.Topology as the dict count_all returns."""
    out = dict((name, int(getattr(t, name))) for name in
               ("numVertices", "numTriangles", "duplicateEdges", "boundaryEdges", "edges", "numComponents", "numBoundaries",
                "eulerCharacteristic", "firstIndex", "firstKind", "manifold"))
    out["count"] = [int(x) for x in t.count]
    out["firstOf"] = [int(x) for x in t.firstOf]
    return out


_VERDICTS = [(re.compile(r"Triangle (\d+) contains out-of-range index"), OUT_OF_RANGE),
             (re.compile(r"Triangle (\d+) contains vertex \d+ twice"), DEGENERATE),
             (re.compile(r"Vertex (\d+) is isolated"), ISOLATED),
             (re.compile(r"Edge (\d+) - (\d+) occurs twice"), DUPLICATED),
             (re.compile(r"Vertex (\d+) is both in the interior and on the boundary"), MIXED),
             (re.compile(r"Vertex (\d+) tunnels between interior regions"), TUNNEL)]


def verdict_of(message):
    """(class, index) that a message of refdata.is_manifold names; the index of a DUPLICATED edge is None (the
    reference names the edge at whichever end it visits first)."""
    if message == "":
        return NONE, None
    for pattern, kind in _VERDICTS:
        m = pattern.match(message)
        if m:
            return kind, (None if kind == DUPLICATED else int(m.group(1)))
    raise AssertionError(message)


# ---------------------------------------------------------------- meshes

def torus(n, m):
    """n x m vertices on a torus, two triangles per quad: closed, one component, Euler characteristic 0 (n, m >= 3)."""
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    v00, v10 = i * m + j, (i + 1) % n * m + j
    v01, v11 = i * m + (j + 1) % m, (i + 1) % n * m + (j + 1) % m
    return n * m, np.concatenate([np.stack([v00, v10, v11], axis=-1).reshape(-1, 3),
                                  np.stack([v00, v11, v01], axis=-1).reshape(-1, 3)]).astype(np.int64)


def grid(n, m):
    """An open sheet of n x m vertices: one component, one boundary of 2 (n - 1) + 2 (m - 1) edges, Euler 1."""
    i, j = np.meshgrid(np.arange(n - 1), np.arange(m - 1), indexing="ij")
    v00, v10, v01, v11 = i * m + j, (i + 1) * m + j, i * m + j + 1, (i + 1) * m + j + 1
    tri = np.stack([np.stack([v00, v10, v11], axis=-1), np.stack([v00, v11, v01], axis=-1)], axis=2)
    return n * m, tri.reshape(-1, 3).astype(np.int64)          # the two triangles of a quad side by side


def cone(n, hub=0, first=1):
    """n triangles around `hub` over the ring of vertices first .. first + n - 1: a disc, the hub in its interior."""
    ring = first + np.arange(n)
    return np.stack([np.full(n, hub), ring, first + (np.arange(n) + 1) % n], axis=1).astype(np.int64)


def random_mesh(rng):
    """A 3..6 x 3..6 torus with 0..4 edits out of seven kinds; returns (V, triangles), indices below V + 2."""
    V, tri = torus(int(rng.integers(3, 7)), int(rng.integers(3, 7)))
    tri = tri.copy()
    for _ in range(int(rng.integers(0, 5))):
        edit = int(rng.integers(0, 7))
        if len(tri) == 0:
            break
        t = int(rng.integers(0, len(tri)))
        if edit == 0:                                       # drop a triangle
            tri = np.delete(tri, t, axis=0)
        elif edit == 1:                                     # repeat one
            tri = np.concatenate([tri, tri[t:t + 1]])
        elif edit == 2:                                     # flip one
            tri[t] = tri[t][[0, 2, 1]]
        elif edit == 3:                                     # overwrite an index, possibly out of range
            tri[t, int(rng.integers(0, 3))] = int(rng.integers(0, V + 2))
        elif edit == 4:                                     # a vertex nothing uses
            V += 1
        elif edit == 5:                                     # merge two vertices
            a, b = (int(x) for x in rng.integers(0, V, 2))
            tri[tri == b] = a
        else:                                               # delete a vertex's star
            v = int(rng.integers(0, V))
            tri = tri[~(tri == v).any(axis=1)]
    return V, tri


def classification_trap():
    """(vertices, triangles): a unit square of two triangles and three bad ones on which the stages disagree BY CONTRACT.  The
    topology report takes the first failing check of the reference's rotation order (i0 >= V, i0 == i1, i1 >= V, i1 == i2,
    i2 >= V, i2 == i0); smoothing and hole filling look at the range of all three indices first.  So (1, 1, 7) is degenerate
    for the one and out of range for the others; (7, 2, 2) is out of range and (3, 3, 3) degenerate for all of them."""
    p = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    return p, np.array([[0, 1, 2], [0, 2, 3], [1, 1, 7], [7, 2, 2], [3, 3, 3]], np.int64)


def assert_trap_report(r):
    """What the topology report says of classification_trap()."""
    assert r["count"][:2] == [1, 2] and r["firstOf"][:2] == [3, 2] and (r["firstKind"], r["firstIndex"]) == (DEGENERATE, 2), r
    assert (r["manifold"], r["boundaryEdges"], r["duplicateEdges"]) == (0, 4, 0), r
