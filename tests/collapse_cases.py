"""A CPU oracle for the short-edge collapse (mlsgpu_hip_mesh_collapse_edges), and the meshes its tests share.

collapse() follows the contract in include/mlsgpu_hip.h step by step, a round at a time: np.unique on the directed sides for the
runs, float64 arrays for the lengths and the fold test -- every numpy operation is one correctly rounded double operation,
written in the contract's order --, plain Python sets for the link condition of the few short edges, and np.minimum.at for the
choice of a round.  Nothing here is product code.
"""
import numpy as np

from flip_cases import Invalid, classes, dot, face, quality, renumbered, triangle_set  # noqa: F401  (the tests use them)
from simplify_cases import grid_mesh

MIN_COS = 0.5
MAX_VALENCE = 64
STAT_NAMES = ("numVertices", "numTriangles", "outOfRangeTriangles", "degenerateTriangles", "numEdges", "interiorEdges",
              "fixedVertices", "rounds", "collapses", "converged", "shortBefore", "shortAfter", "blockedAfter", "unusedVertices",
              "outVertices", "outTriangles", "minQualityBefore", "minQualityAfter", "minLengthSqBefore", "minLengthSqAfter",
              "qualityBefore", "qualityAfter")
U32 = np.uint64(32)


def empty_stats():
    out = dict.fromkeys(STAT_NAMES, 0)
    out.update(minQualityBefore=0.0, minQualityAfter=0.0, minLengthSqBefore=np.inf, minLengthSqAfter=np.inf,
               qualityBefore=[0] * 16, qualityAfter=[0] * 16)
    return out


def classify(p, tri, live, limit, min_cos):
    """Steps 2 to 6 on the current triangles: the counts, and per candidate its a, b, L2, survivor, removed vertex, new
    position (float32) and S; `at` gives the (row, corner) pairs of the triangles at a vertex."""
    V = len(p)
    slots = np.flatnonzero(live)
    t = tri[live]
    src, dst, opp = t.ravel(), t[:, [1, 2, 0]].ravel(), t[:, [2, 0, 1]].ravel()
    slot, corner = np.repeat(slots, 3), np.tile(np.arange(3), len(t))
    key = src.astype(np.uint64) << U32 | dst.astype(np.uint64)
    sides, first, uses = np.unique(key, return_index=True, return_counts=True)
    num_edges = len(np.unique(np.minimum(src, dst).astype(np.uint64) << U32 | np.maximum(src, dst).astype(np.uint64)))
    a, b = sides >> U32, sides & np.uint64(0xFFFFFFFF)
    back = np.searchsorted(sides, b << U32 | a)
    back[back == len(sides)] = 0
    twin = sides[back] == (b << U32 | a) if len(sides) else np.zeros(0, bool)
    fixed = np.zeros(V, bool)                                   # step 2
    loose = (uses > 1) | ~twin
    fixed[a[loose].astype(np.int64)] = True
    fixed[b[loose].astype(np.int64)] = True
    regular = (a < b) & (uses == 1) & twin & (uses[back] == 1) if len(sides) else np.zeros(0, bool)
    i, j = first[regular], first[back[regular]]
    a, b, c, d = a[regular].astype(np.int64), b[regular].astype(np.int64), opp[i], opp[j]
    keep = c != d                                               # step 3
    a, b, c, d, t1, t2 = a[keep], b[keep], c[keep], d[keep], slot[i][keep], slot[j][keep]
    e = p[b] - p[a]
    L2 = dot(e, e)                                              # step 4
    short = L2 <= limit
    counts = dict(numEdges=num_edges, interiorEdges=len(a), fixedVertices=int(fixed.sum()), short=int(short.sum()),
                  minLengthSq=float(L2.min()) if len(L2) else np.inf)
    a, b, c, d, t1, t2, L2 = [x[short] for x in (a, b, c, d, t1, t2, L2)]
    n = len(a)
    order = np.argsort(src, kind="stable")
    start = np.searchsorted(src[order], np.arange(V + 1))

    def at(x):
        return order[start[x]:start[x + 1]]

    side_set = set(sides.tolist()) if n else set()
    both = fixed[a] & fixed[b]
    survivor = np.where(fixed[b] & ~fixed[a], b, a)             # step 5
    removed = a + b - survivor
    middle = ((p[a] + p[b]) * 0.5).astype(np.float32)
    new32 = np.where((fixed[a] | fixed[b])[:, None], p[survivor].astype(np.float32), middle)
    blocked = both.copy()                                       # guard (i)
    S = [None] * n
    fold = []                                                   # (edge, x, q, r): the triangle (x, q, r) holds x = a or b
    for k in range(n):
        ra, rb = at(a[k]), at(b[k])
        if len(ra) > MAX_VALENCE or len(rb) > MAX_VALENCE:      # guard (ii)
            blocked[k] = True
            continue
        Na = set(dst[ra].tolist()) | set(opp[ra].tolist())
        Nb = set(dst[rb].tolist()) | set(opp[rb].tolist())
        if Na & Nb != {int(c[k]), int(d[k])}:                   # guard (iii)
            blocked[k] = True
        if (int(c[k]) << 32 | int(d[k])) in side_set or (int(d[k]) << 32 | int(c[k])) in side_set:     # guard (iv)
            blocked[k] = True
        S[k] = sorted({int(a[k]), int(b[k])} | Na | Nb)
        for r in np.concatenate([ra, rb]).tolist():
            if slot[r] != t1[k] and slot[r] != t2[k]:
                fold.append((k, src[r], dst[r], opp[r]))
    if fold:                                                    # guard (v)
        k, x, q, r = np.array(fold, np.int64).T
        new = new32.astype(np.float64)[k]
        n0, n1 = face(p[x], p[q], p[r]), face(new, p[q], p[r])
        with np.errstate(invalid="ignore"):
            ok = (dot(n0, n1) > 0) & (dot(n0, n1) >= (min_cos * np.sqrt(dot(n0, n0))) * np.sqrt(dot(n1, n1)))
        fails = (dot(n0, n0) != 0) & ~ok
        blocked[np.unique(k[fails])] = True
    counts["blocked"] = int(blocked.sum())
    cand = np.flatnonzero(~blocked)
    rows = dict((int(x), (slot[at(x)], corner[at(x)])) for x in removed[cand])
    return counts, dict(a=a[cand], b=b[cand], L2=L2[cand], survivor=survivor[cand], removed=removed[cand], new=new32[cand],
                        S=[S[k] for k in cand], rows=rows)


def winners(num_vertices, a, b, L2, S):
    """Step 7: the mask of the candidates that win."""
    key = a.astype(np.uint64) << U32 | b.astype(np.uint64)     # ordered as a << bitLength(V) | b is
    who = np.repeat(np.arange(len(S)), [len(s) for s in S])
    v = np.array([x for s in S for x in s], np.int64)
    best = np.full(num_vertices, np.inf)
    np.minimum.at(best, v, L2[who])
    least = np.full(num_vertices, np.iinfo(np.uint64).max, np.uint64)
    holds = L2[who] == best[v]
    np.minimum.at(least, v[holds], key[who][holds])
    lost = np.zeros(len(S), bool)
    lost[who[~(holds & (key[who] == least[v]))]] = True
    return ~lost


def collapse(vertices, triangles, max_rounds, max_length, min_cos=MIN_COS, trace=None):
    """(vertices float32 [V', 3], triangles uint32 [T', 3], statistics dict, source uint32 [V']) or Invalid.  `trace`, a list,
    gets one dict per round: its candidates, its winners, and whether two of its candidates have the same L2."""
    p32 = np.array(vertices, np.float32).reshape(-1, 3)
    tri = np.array(triangles, np.int64).reshape(-1, 3) & 0xFFFFFFFF
    if not (np.isfinite(max_length) and max_length >= 0 and 0 <= min_cos <= 1):
        raise Invalid("parameters")
    if not np.isfinite(p32).all():
        raise Invalid("vertex")
    limit = np.float64(max_length) * np.float64(max_length)
    p, V = p32.astype(np.float64), len(p32)
    stats = empty_stats()
    stats.update(numVertices=V, numTriangles=len(tri))
    out_of_range, degenerate = classes(V, tri)
    live = ~out_of_range & ~degenerate
    stats.update(outOfRangeTriangles=int(out_of_range.sum()), degenerateTriangles=int(degenerate.sum()))
    stats["minQualityBefore"], stats["qualityBefore"] = quality(p, tri, live)
    first = True
    while True:                                                 # step 9
        counts, c = classify(p, tri, live, limit, min_cos)
        if first:
            stats.update(numEdges=counts["numEdges"], interiorEdges=counts["interiorEdges"], fixedVertices=counts["fixedVertices"],
                         shortBefore=counts["short"], minLengthSqBefore=counts["minLengthSq"])
            first = False
        stats.update(shortAfter=counts["short"], blockedAfter=counts["blocked"], minLengthSqAfter=counts["minLengthSq"])
        if stats["rounds"] == max_rounds:
            break
        stats["rounds"] += 1
        win = winners(V, c["a"], c["b"], c["L2"], c["S"]) if len(c["a"]) else np.zeros(0, bool)
        if trace is not None:
            trace.append(dict(candidates=len(win), winners=int(win.sum()), ties=len(np.unique(c["L2"])) != len(win)))
        assert win.any() == (len(win) > 0)
        if not win.any():
            stats["converged"] = 1
            break
        stats["collapses"] += int(win.sum())
        for k in np.flatnonzero(win):                           # step 8
            rows, corners = c["rows"][int(c["removed"][k])]
            tri[rows, corners] = c["survivor"][k]
            p32[c["survivor"][k]] = c["new"][k]
        p = p32.astype(np.float64)
        live = live & ~((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 2] == tri[:, 0]))
    stats["minQualityAfter"], stats["qualityAfter"] = quality(p, tri, live)
    used = np.zeros(V, bool)                                    # step 10
    used[tri[live].ravel()] = True
    source = np.flatnonzero(used)
    number = np.cumsum(used) - 1
    out_tri = number[tri[live]].astype(np.uint32).reshape(-1, 3)
    stats.update(unusedVertices=V - len(source), outVertices=len(source), outTriangles=len(out_tri))
    return p32[source], out_tri, stats, source.astype(np.uint32)


def assert_same(got, want):
    """(vertices, triangles, stats[, source]) against the oracle's: every bit, every row and every statistic exactly."""
    assert got[2] == want[2], (got[2], want[2])
    gv, wv = np.ascontiguousarray(got[0], np.float32).reshape(-1, 3), np.ascontiguousarray(want[0], np.float32).reshape(-1, 3)
    assert gv.shape == wv.shape and gv.tobytes() == wv.tobytes()
    gt = np.ascontiguousarray(got[1], np.uint32).reshape(-1, 3)
    assert gt.shape == want[1].shape
    np.testing.assert_array_equal(gt, want[1])
    if len(got) > 3:
        np.testing.assert_array_equal(np.asarray(got[3], np.uint32).ravel(), want[3])


def invariants(num_vertices, triangles):
    """What a collapse keeps of topology_cases.count_all's report."""
    import topology_cases as tc
    r = tc.count_all(num_vertices, np.asarray(triangles, np.int64).reshape(-1, 3))
    return dict((name, r[name]) for name in ("manifold", "numComponents", "numBoundaries", "boundaryEdges", "eulerCharacteristic"))


# ---------------------------------------------------------------- meshes

def disk(ring=8, pair=0.01, rim=False):
    """A flat disk: vertices 0 = (-pair / 2, 0) and 1 = (pair / 2, 0), a ring of `ring` vertices (a multiple of 4) at radius 1
    around them, of which 0 sees the left half and 1 the right one, and a second ring at radius 2, so that 0 and 1 are
    interior and the edge 0 1 is the only short one.  With `rim` there is no second ring and no triangle (1, ring 0, ring 1):
    a notch, at whose tip vertex 1 lies on the boundary."""
    a = 2 * np.pi * np.arange(ring) / ring
    inner = np.stack([np.cos(a), np.sin(a), np.zeros(ring)], axis=1)
    q = ring // 4

    def R(k):
        return 2 + k % ring

    def Q(k):
        return 2 + ring + k % ring

    tri = [[0, 1, R(q)], [1, 0, R(3 * q)]]
    tri += [[1, R(k), R(k + 1)] for k in range(3 * q, 5 * q)]
    tri += [[0, R(k), R(k + 1)] for k in range(q, 3 * q)]
    p = np.concatenate([[[-pair / 2, 0, 0], [pair / 2, 0, 0]], inner])
    if rim:
        tri.remove([1, R(0), R(1)])
        return p.astype(np.float32), np.array(tri, np.int64)
    outer = 2 * np.stack([np.cos(a + np.pi / ring), np.sin(a + np.pi / ring), np.zeros(ring)], axis=1)
    tri += [[R(k), Q(k), R(k + 1)] for k in range(ring)] + [[R(k), Q(k - 1), Q(k)] for k in range(ring)]
    return np.concatenate([p, outer]).astype(np.float32), np.array(tri, np.int64)


def tube(rings=6, side=0.017, spacing=1.0):
    """A triangular tube with open ends: ring i has three vertices 3 i + j, `side` apart, at z = i * spacing.  The ring edges of
    the inner rings are short, and collapsing one would pinch the tube: N(a) and N(b) share the ring's third vertex."""
    r = side / np.sqrt(3.0)
    a = 2 * np.pi * np.arange(3) / 3
    p = np.concatenate([np.stack([r * np.cos(a), r * np.sin(a), np.full(3, i * spacing)], axis=1) for i in range(rings)])
    tri = []
    for i in range(rings - 1):
        for j in range(3):
            u, v = 3 * i + j, 3 * i + (j + 1) % 3
            tri += [[u, v, u + 3], [v, v + 3, u + 3]]
    return p.astype(np.float32), np.array(tri, np.int64)


def star():
    """disk() with ring vertex 2 (index 4) pulled in to (0.01659, 0.01414), onto a line from ring vertex 1 that meets the x axis
    at 0.0025: the collapse carries vertex 1 from (0.005, 0) to the midpoint (0, 0) across that line, and the triangle
    (1, 3, 4) would turn over."""
    p, tri = disk(8, 0.01)
    p = p.copy()
    p[4] = [0.01659, 0.01414, 0.0]
    return p, tri


def coincident():
    """disk() with vertices 0 and 1 on the same spot."""
    p, tri = disk(8, 0.01)
    p = p.copy()
    p[1] = p[0]
    return p, tri


def needle_row(n=12, m=30, count=20, gap=0.01):
    """grid_mesh(n, m) whose row n // 2 has `count` vertices in a line only `gap` apart (columns 5 .. 5 + count): a chain of
    short edges, of which a round can take only every third or so."""
    p, tri = grid_mesh(n, m)
    p = p.copy()
    i = n // 2
    for k in range(count):
        p[i * m + 5 + k, 1] = 5 + count / 2 + (k - count / 2) * gap
    return p, tri


def planted_needles(seed=5):
    """grid_mesh(40, 40, 0.1, 2) with vertex (i, j), i, j in 2, 7, ..., 37, moved to within 1e-3 of vertex (i + 1, j): 64 needles."""
    p, tri = grid_mesh(40, 40, 0.1, 2)
    p = p.astype(np.float64)
    rng = np.random.default_rng(seed)
    for i in range(2, 40, 5):
        for j in range(2, 40, 5):
            step = rng.normal(size=3)
            p[i * 40 + j] = p[(i + 1) * 40 + j] + step / np.linalg.norm(step) * rng.uniform(2e-4, 1e-3) * [1, 1, 0]
    return p.astype(np.float32), tri


def defect_mesh():
    """A jittered grid with a triangle that names vertex 0xFFFFFFFF, one that names V, two degenerate triangles and two unused
    vertices."""
    p, tri = grid_mesh(9, 11, 0.45, 3)
    p = np.concatenate([p, [[4.0, 4.0, 1.0], [-2.0, 0.5, 0.25]]]).astype(np.float32)
    tri = tri.copy()
    tri[5, 2] = len(p)
    tri[77, 0] = 0xFFFFFFFF
    tri[20, 1] = tri[20, 0]
    tri[121, 2] = tri[121, 1]
    return p, tri
