"""Inputs and a numpy model for chains of stages on one device sink (csrc/mesher.hip: simplifyChunks, stageInPlace,
stageIntoNewGeneration; mlsgpu::seamMask in csrc/fill.hip): tests/test_sink_chain_oracle.py checks on the CPU what
tests/test_gpu_sink_chain.py relies on.

The sheet: 49 x 49 vertices, grid vertex (i, j) at (i - 20 + jx, j + jy, 2 sin(0.3 i) cos(0.23 j)) with jx, jy uniform in
+-0.25 (seed 7), two triangles per cell, cut into 3 x 3 tiles of 16 x 16 cells; tile t = 3 ty + tx.  The vertices on the
two inner cut lines of either direction are external, with sink_cases.sheet_key(i, j); single cells are missing, four
inside tiles and one on either side of a seam edge.  The shift by -20 puts grid column 20, which is inside tile column 1, at x = 0: vertex
ZERO_AT = (20, 5) has its x set to -0.0 in every variant, and `twins` gives tile 0 a vertex with +0.0 and the same y and z.
A mesh is the dict of sink_cases.py: chunk, vertices (internal first), num_internal, keys, triangles."""
import copy

import numpy as np

import collapse_cases as cc
import deviation_cases as dc
import fill_cases as fc
import flip_cases as fl
import intersect_cases as ic
import repair_cases as rc
import simplify_cases as sc
import simplify_quadric_cases as sq
import smooth_cases as sm
import split_cases as sp
from sink_cases import mo, sheet_key

N, TILE, SHIFT_X, ZERO_AT = 48, 16, -20.0, (20, 5)
# cells (i, j): one inside each of tiles 0, 4, 8 and 6, and the two cells on either side of the seam edge (32, 8)-(32, 9): a
# single cell against the seam in tile 1 and in tile 2, so that neither holds the edge and the seam starts closed
HOLES = ((5, 5), (24, 24), (40, 40), (10, 37), (31, 8), (32, 8))
QUIET_CELL = (24, 24)           # gaps: the chunk without triangles holds the corners of this hole
GAP_IDS = (70, 3, 41, 9, 1000000007, 12, 5, 88, 2)              # gaps: the caller's id of tile t
QUIET_ID, ISLAND_ID = 55, 4
TWIN_SEAM, TWIN_INNER = (16, 20), (20, 40)                      # twins (a): held by tiles 3 and 4; (b): inside tile 7

# the parameters of the chains (the issue's; see test_sink_chain_oracle.py for what they have to satisfy)
MAX_ROUNDS, FILL_EDGES, SPLIT_LENGTH, COLLAPSE_LENGTH, SMOOTH_PASSES = 64, 32, 0.8, 0.45, 3
SIMPLIFY_CELL, QUADRIC_CELL, DEVIATION = 2.5, 5.0, 0.75
SIMPLIFY_ORIGIN = (-22.5, -2.5, -5.0)
EMPTY_ORIGIN, EMPTY_CELL = (-24.0, -4.0, -8.0), 64.0            # one cell holds the whole sheet


# ---------------------------------------------------------------- the inputs

def sheet():
    """float32 [49, 49, 3]: the position of grid vertex (i, j)."""
    i, j = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    jitter = np.random.default_rng(7).uniform(-0.25, 0.25, (N + 1, N + 1, 2))
    p = np.stack([i + SHIFT_X + jitter[..., 0], j + jitter[..., 1], 2.0 * np.sin(0.3 * i) * np.cos(0.23 * j)], axis=-1).astype(np.float32)
    p[ZERO_AT][0] = np.float32(-0.0)
    return p


def cut_lines():
    """bool [49, 49]: the grid vertices on the inner cut lines."""
    i, j = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    return ((i % TILE == 0) & (i > 0) & (i < N)) | ((j % TILE == 0) & (j > 0) & (j < N))


def tile_cells(t, keep=lambda i, j: True):
    """The cells (i, j) of tile t that are no holes and that `keep` admits, as an [n, 2] array in row-major order."""
    tx, ty = t % 3, t // 3
    return np.array([(i, j) for i in range(TILE * tx, TILE * tx + TILE) for j in range(TILE * ty, TILE * ty + TILE)
                     if (i, j) not in HOLES and keep(i, j)], np.int64).reshape(-1, 2)


def block(chunk, cells, P, external):
    """One block of the cells' triangles ((a, b, c) and (a, c, d) around the cell, counter-clockwise seen from +z): the
    vertices they use, internal ones first and each kind in ascending (i, j); `external` is a bool [49, 49]."""
    i, j = cells[:, 0], cells[:, 1]
    stride = N + 1
    a, b, c, d = i * stride + j, (i + 1) * stride + j, (i + 1) * stride + j + 1, i * stride + j + 1
    tri = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], axis=1).reshape(-1, 3)
    used = np.unique(tri)
    ext = external.reshape(-1)[used]
    used = used[np.lexsort((used, ext))]
    ext = external.reshape(-1)[used]
    local = np.zeros(stride * stride, np.int64)
    local[used] = np.arange(len(used))
    return dict(chunk=chunk, vertices=P.reshape(-1, 3)[used].copy(), num_internal=int((~ext).sum()),
                keys=sheet_key(used[ext] // stride, used[ext] % stride), triangles=local[tri].astype(np.uint32))


def loose(chunk, vertices, triangles):
    """A block of internal vertices only."""
    return dict(chunk=chunk, vertices=np.asarray(vertices, np.float32).reshape(-1, 3), num_internal=len(vertices),
                keys=np.zeros(0, np.uint64), triangles=np.asarray(triangles, np.uint32).reshape(-1, 3))


def tiles():
    P, external = sheet(), cut_lines()
    return [block(t, tile_cells(t), P, external) for t in range(9)]


def gaps():
    """Every tile in two blocks (rows j % 16 < 8 and the rest, the line between them external too), the first halves in tile
    order with the chunk without triangles arriving 2nd and the island 5th, then the second halves in another order.  The
    chunk without triangles holds the four corners of hole QUIET_CELL, which tile 4 declares external: they weld to the
    sheet, so finalize keeps them in a dense chunk that has no output, and the seam mask pins tile 4's copies."""
    P, external = sheet(), cut_lines()
    i, j = np.meshgrid(np.arange(N + 1), np.arange(N + 1), indexing="ij")
    external |= j % 8 == 0
    qi, qj = QUIET_CELL
    corners = np.array([(qi, qj), (qi + 1, qj), (qi + 1, qj + 1), (qi, qj + 1)])
    external[corners[:, 0], corners[:, 1]] = True
    lower = [block(GAP_IDS[t], tile_cells(t, lambda i, j: j % TILE < 8), P, external) for t in range(9)]
    upper = [block(GAP_IDS[t], tile_cells(t, lambda i, j: j % TILE >= 8), P, external) for t in range(9)]
    quiet = dict(chunk=QUIET_ID, vertices=P[corners[:, 0], corners[:, 1]].copy(), num_internal=0,
                 keys=sheet_key(corners[:, 0], corners[:, 1]), triangles=np.zeros((0, 3), np.uint32))
    island = loose(ISLAND_ID, [[0, 0, 30], [1, 0, 30], [1, 1, 30.5], [0, 1, 30], [-1, 0.5, 30]], [[0, 1, 2], [0, 2, 3], [0, 3, 4]])
    return [lower[0], quiet, lower[1], lower[2], island] + lower[3:] + [upper[t] for t in (5, 0, 8, 3, 1, 7, 2, 6, 4)]


def gaps_prune():
    """The prune fraction of `gaps`: a threshold of 6 welded vertices, which only the island (5) misses."""
    return 6.5 / (49 * 49 + 5)


def with_fan(mesh, at):
    """`mesh` with four more internal vertices -- one at `at`, three above it -- and the two triangles of a fan around the first;
    returns the mesh and the index of the vertex at `at`."""
    at = np.asarray(at, np.float32)
    ni = mesh["num_internal"]
    more = np.stack([at, at + np.float32([1, 0, 3]), at + np.float32([1, 1, 3.5]), at + np.float32([0, 1, 3])]).astype(np.float32)
    more[0] = at                                                    # the bits of `at`, a zero's sign included
    tri = mesh["triangles"].astype(np.int64)
    tri = np.where(tri >= ni, tri + 4, tri)
    out = dict(mesh, vertices=np.concatenate([mesh["vertices"][:ni], more, mesh["vertices"][ni:]]), num_internal=ni + 4,
               triangles=np.concatenate([tri, [[ni, ni + 1, ni + 2], [ni, ni + 2, ni + 3]]]).astype(np.uint32))
    return out, ni


def twins():
    """tiles with (a) in tile 4 a vertex at the 12 bytes of seam vertex TWIN_SEAM, which tile 3 holds too, (b) in tile 7 a
    second vertex at the 12 bytes of its vertex TWIN_INNER, (c) in tile 0 a vertex at (+0.0, y, z) where tile 1's vertex ZERO_AT
    lies at (-0.0, y, z).  Returns (meshes, {"a" | "b" | "c": (tile, index of the new vertex in its block)})."""
    P, meshes, where = sheet(), tiles(), {}
    zero = P[ZERO_AT].copy()
    zero[0] = np.float32(0.0)
    for name, t, at in (("a", 4, P[TWIN_SEAM]), ("b", 7, P[TWIN_INNER]), ("c", 0, zero)):
        meshes[t], index = with_fan(meshes[t], at)
        where[name] = (t, index)
    return meshes, where


def crumb():
    """tiles and a tenth chunk: 3 x 3 vertices half a unit apart, all inside one simplify cell of SIMPLIFY_CELL, far above the sheet."""
    base = np.float32(SIMPLIFY_ORIGIN) + np.float32(SIMPLIFY_CELL) * np.float32([4, 4, 8]) + np.float32([0.6, 0.6, 1.0])
    i, j = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    v = base + np.stack([0.5 * i, 0.5 * j, 0.05 * i * j], axis=-1).reshape(-1, 3).astype(np.float32)
    q = np.array([(a * 3 + b) for a in range(2) for b in range(2)])
    tri = np.stack([np.stack([q, q + 3, q + 4], 1), np.stack([q, q + 4, q + 1], 1)], axis=1).reshape(-1, 3)
    return tiles() + [loose(9, v, tri)]


def variant(name):
    """(meshes, prune fraction) of tiles, gaps, twins or crumb."""
    if name == "gaps":
        return gaps(), gaps_prune()
    return {"tiles": tiles, "twins": lambda: twins()[0], "crumb": crumb}[name](), 0.0


def rows12(vertices):
    """The 12 bytes of every vertex, as uint32 [n, 3]."""
    return np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).view(np.uint32)


def quiet_chunks(meshes, prune):
    """What finalize keeps of the dense chunks that get no output: {dense index: (caller's id, vertices)}.  A vertex stays if it
    is the first of its key in its chunk and its component has at least uint64(total * prune) welded vertices (the rule of
    mesher_oracle.mesh_sink), in the order (arrival within the chunk, index within the block)."""
    L = mo.mesh_sink_labels(meshes)
    n = len(L["comp_rep"])
    pos = np.concatenate([np.asarray(meshes[i]["vertices"], np.float32).reshape(-1, 3) for i in L["order"]])
    chunk_of_vertex = np.repeat(L["chunk_of"], np.diff(L["bases"]))
    rep = L["comp_rep"] == np.arange(n)
    size = np.bincount(L["label"][rep], minlength=int(L["label"].max()) + 1)
    keep = size[L["label"]] >= int(np.uint64(int(rep.sum()) * prune))
    chunk_of_triangle = chunk_of_vertex[L["triangles"][:, 0]]
    kept_triangles = np.bincount(chunk_of_triangle[keep[L["triangles"][:, 0]]], minlength=len(L["chunks"]))
    out = {}
    for c, cid in enumerate(L["chunks"]):
        if kept_triangles[c] == 0:
            out[c] = (cid, pos[(chunk_of_vertex == c) & (L["out_rep"] == np.arange(n)) & keep])
    return out


# ---------------------------------------------------------------- the model

def seam_masks(vertex_arrays):
    """The documented rule of mlsgpu::seamMask for n chunks: per chunk a bool per vertex, set iff a DIFFERENT chunk holds a vertex
    with the same 12 bytes -- the chunks per row are counted, not the vertices per row."""
    rows = np.concatenate([rows12(v) for v in vertex_arrays]) if vertex_arrays else np.zeros((0, 3), np.uint32)
    chunk = np.repeat(np.arange(len(vertex_arrays)), [len(v) for v in vertex_arrays])
    if len(rows) == 0:
        return [np.zeros(0, bool) for _ in vertex_arrays]
    _, row_id = np.unique(rows, axis=0, return_inverse=True)
    row_id = row_id.reshape(-1)
    pairs = np.unique(row_id * len(vertex_arrays) + chunk)          # one entry per (row, chunk that holds it)
    holders = np.bincount(pairs // len(vertex_arrays), minlength=int(row_id.max()) + 1)
    pinned = holders[row_id] > 1
    return [pinned[chunk == c] for c in range(len(vertex_arrays))]


def summed_simplify(stats):
    return dict((name, sum(st[name] for st in stats)) for name in sc.STAT_NAMES)


def summed_quadric(stats):
    """The counts add; scaleExponent is the largest among the chunks that have a scale (where a vertex solved or escaped)."""
    out = dict((name, sum(st[name] for st in stats)) for name in sq.STAT_NAMES if name != "scaleExponent")
    scaled = [st["scaleExponent"] for st in stats if st["solvedVertices"] + st["escapedVertices"] > 0]
    out["scaleExponent"] = max(scaled) if scaled else 0
    return out


def _empty(n=0):
    return np.zeros((n, 3), np.float32), np.zeros((0, 3), np.uint32)


_MEMORY = {}        # (stage, parameters, the chunk's bytes, its mask) -> the oracle's result: read only


def _remembered(name, oracle, key, *arrays):
    """oracle(*arrays), from _MEMORY where the same report was asked of the same bytes before."""
    memo = (name, repr(key)) + tuple(a.tobytes() for a in arrays)
    if memo not in _MEMORY:
        _MEMORY[memo] = oracle(*arrays)
    return _MEMORY[memo]


class SinkModel:
    """The dense chunks [caller's id, vertices, triangles] of a finalized sink and the dense indices that have output.  One
    method per stage of binding.Mesher, with its arguments: it runs the stage's oracle on every dense chunk that has triangles,
    leaves per dense chunk the oracle's result in self.last (None where the chunk was skipped) and returns the statistics the
    sink reports.  A chunk without triangles: the two routes that write the chunks anew (to the front, into a new generation)
    keep nothing of it; the in-place route leaves it alone, vertices included."""

    def __init__(self, dense, out):
        self.dense = [[cid, np.array(v, np.float32).reshape(-1, 3), np.array(t, np.uint32).reshape(-1, 3)] for cid, v, t in dense]
        self.out = list(out)
        self.original = copy.deepcopy(self.dense)
        self.reference = None
        self.last = [None] * len(self.dense)
        self.rounds = []            # (stage, chunk, rounds, converged) of every split, collapse and flip

    @classmethod
    def from_output(cls, chunks, quiet):
        """chunks: the output chunks (id, vertices, triangles) in order; quiet: quiet_chunks() of the same input."""
        dense, out, chunks = [], [], list(chunks)
        for c in range(len(chunks) + len(quiet)):
            if c in quiet:
                dense.append((quiet[c][0], quiet[c][1], _empty()[1]))
            else:
                out.append(c)
                dense.append(chunks.pop(0))
        return cls(dense, out)

    def chunks(self):
        return [tuple(self.dense[c]) for c in self.out]

    def masks(self):
        """Per dense chunk the pinned vertices, or None where the sink builds no mask: with at most one output chunk."""
        if len(self.out) <= 1:
            return [None] * len(self.dense)
        return seam_masks([d[1] for d in self.dense])

    def _run(self, name, oracle, fold, preset, route, key=(), masks=None):
        """key: the stage's parameters, for the memory of oracle results that the chains share (_MEMORY).  route: "front",
        "generation" (the oracle returns vertices, triangles, statistics, ...), "vertices" or "triangles" (in place: the
        oracle returns that array and the statistics)."""
        ran, self.last = [], [None] * len(self.dense)
        for c, d in enumerate(self.dense):
            if len(d[2]) == 0:
                if route in ("front", "generation"):
                    d[1], d[2] = _empty()
                continue
            memo = (name, repr(key), d[1].tobytes(), d[2].tobytes(), None if masks is None or masks[c] is None else masks[c].tobytes())
            if memo not in _MEMORY:
                _MEMORY[memo] = oracle(c, d[1], d[2])
            want = _MEMORY[memo]
            self.last[c] = want
            if route == "vertices":
                d[1] = np.array(want[0], np.float32).reshape(-1, 3)
            elif route == "triangles":
                d[2] = np.array(want[0], np.uint32).reshape(-1, 3)
            else:
                d[1], d[2] = np.array(want[0], np.float32).reshape(-1, 3), np.array(want[1], np.uint32).reshape(-1, 3)
            st = want[1] if route in ("vertices", "triangles") else want[2]
            if "rounds" in st:
                self.rounds.append((name, c, st["rounds"], st["converged"]))
            ran.append(st)
        return fold(ran) if ran else preset

    def simplify(self, origin, cell):
        return self._run("simplify", lambda c, v, t: sc.simplify(v, t, origin, cell), summed_simplify, dict.fromkeys(sc.STAT_NAMES, 0), "front",
                         (origin, cell))

    def simplify_quadric(self, origin, cell):
        return self._run("simplify_quadric", lambda c, v, t: sq.simplify_quadric(v, t, origin, cell), summed_quadric,
                         dict.fromkeys(sq.STAT_NAMES, 0), "front", (origin, cell))

    def smooth(self, iterations, lam=0.5, mu=-0.53, boundary=sm.FIXED):
        from test_gpu_smooth import summed
        preset = dict(dict.fromkeys(sm.STAT_NAMES, 0), passes=int(iterations) * (2 if mu != 0 else 1))
        return self._run("smooth", lambda c, v, t: sm.smooth(v, t, iterations, lam, mu, boundary), summed, preset, "vertices",
                         (iterations, lam, mu, boundary))

    def flip_edges(self, max_rounds, min_gain=fl.MIN_GAIN, min_cos=fl.MIN_COS):
        from test_gpu_flip import summed
        preset = dict(fl.empty_stats(), converged=1 if max_rounds > 0 else 0)
        return self._run("flip", lambda c, v, t: fl.flip(v, t, max_rounds, min_gain, min_cos), summed, preset, "triangles",
                         (max_rounds, min_gain, min_cos))

    def fill_holes(self, max_edges):
        from test_gpu_fill import summed
        masks = self.masks()
        return self._run("fill", lambda c, v, t: fc.fill(v, t, max_edges, masks[c]), summed, dict.fromkeys(fc.STAT_NAMES, 0), "generation",
                         (max_edges,), masks)

    def repair(self, flags=0):
        from test_gpu_repair import summed
        return self._run("repair", lambda c, v, t: rc.repair(v, t, flags), summed, dict.fromkeys(rc.STAT_NAMES, 0), "generation",
                         (flags,))

    def collapse_edges(self, max_rounds, max_length, min_cos=cc.MIN_COS):
        from test_gpu_collapse import summed
        preset = dict(cc.empty_stats(), converged=1 if max_rounds > 0 else 0)
        return self._run("collapse", lambda c, v, t: cc.collapse(v, t, max_rounds, max_length, min_cos), summed, preset, "generation",
                         (max_rounds, max_length, min_cos))

    def split_edges(self, max_rounds, max_length, max_growth=0):
        from test_gpu_split import summed
        masks = self.masks()
        preset = dict(sp.empty_stats(), converged=1 if max_rounds > 0 else 0)
        return self._run("split", lambda c, v, t: sp.split(v, t, max_rounds, max_length, max_growth * len(t), masks[c]), summed, preset,
                         "generation", (max_rounds, max_length, max_growth), masks)

    def finalize(self):
        """Back to the chunks finalize made; a kept reference stays (the chunk list is the same).  Returns the output chunks."""
        self.dense = copy.deepcopy(self.original)
        self.last = [None] * len(self.dense)
        return len(self.out)

    def keep_reference(self):
        self.reference = [(d[1].copy(), d[2].copy()) for d in self.dense]

    def drop_reference(self):
        self.reference = None

    def deviation(self, D):
        """(moved, lost): deviation_cases.deviation per dense chunk in both directions, folded with deviation_cases.combined."""
        assert self.reference is not None
        moved = dc.combined([_remembered("deviation", lambda *a: dc.deviation(*a, D)[2], D, d[1], k[0], k[1]) for d, k in zip(self.dense, self.reference)])
        lost = dc.combined([_remembered("deviation", lambda *a: dc.deviation(*a, D)[2], D, k[0], d[1], d[2]) for d, k in zip(self.dense, self.reference)])
        return moved, lost

    def self_intersections(self):
        return ic.combined([_remembered("intersect", lambda *a: ic.self_intersections(*a)[2], None, d[1], d[2]) for d in self.dense])


def assert_chunk(stage, got_v, got_t, want):
    """A chunk the sink serves behind `stage` against the oracle's result for it, through the stage's own assert_same: the
    statistics slot takes the oracle's, since the sink reports sums (compared apart)."""
    if stage in ("smooth",):
        sm.assert_same((got_v, want[1]), want)
    elif stage in ("flip_edges",):
        fl.assert_same((got_t, want[1]), want)
    else:
        module = dict(simplify=sc, simplify_quadric=sq, fill_holes=fc, repair=rc, collapse_edges=cc, split_edges=sp)[stage]
        module.assert_same((got_v, got_t, want[2]), want[:3])


def open_seams(chunks):
    """The pairs (i, j) of chunks (id, vertices, triangles) that share at least two positions and whose edges between shared
    positions differ: seam_edges of test_gpu_flip.py, over the 12-byte rows both hold.  Empty where every seam is closed."""
    from test_gpu_fill import rows_of
    from test_gpu_flip import seam_edges
    rows = [rows_of(v) for _, v, _ in chunks]
    out = []
    for i in range(len(chunks)):
        for j in range(i + 1, len(chunks)):
            shared = rows[i] & rows[j]
            if len(shared) >= 2 and (seam_edges(dict(vertices=chunks[i][1], triangles=chunks[i][2]), shared)
                                     != seam_edges(dict(vertices=chunks[j][1], triangles=chunks[j][2]), shared)):
                out.append((i, j))
    return out


# ---------------------------------------------------------------- the chains: (method, arguments, R: check every report)
# S2 and S3 begin with a keep_reference beyond the issue's list, so that their deviation reports have something to measure.

R = True
S1_STAGES = [("fill_holes", (FILL_EDGES,), R), ("split_edges", (MAX_ROUNDS, SPLIT_LENGTH), R), ("collapse_edges", (MAX_ROUNDS, COLLAPSE_LENGTH), False),
             ("flip_edges", (MAX_ROUNDS,), False), ("smooth", (SMOOTH_PASSES,), R)]
S1 = ([("keep_reference", (), False)] + S1_STAGES
      + [("split_edges", (MAX_ROUNDS, SPLIT_LENGTH), False), ("keep_reference", (), False), ("collapse_edges", (MAX_ROUNDS, COLLAPSE_LENGTH), R),
         ("finalize", (), False)] + S1_STAGES)
S2 = [("keep_reference", (), False), ("simplify", (SIMPLIFY_ORIGIN, SIMPLIFY_CELL), R), ("repair", (0,), False), ("repair", (rc.SPLIT_PINCHES,), R),
      ("fill_holes", (FILL_EDGES,), False), ("flip_edges", (MAX_ROUNDS,), False), ("split_edges", (MAX_ROUNDS, SPLIT_LENGTH), R),
      ("simplify_quadric", (SIMPLIFY_ORIGIN, QUADRIC_CELL), False), ("collapse_edges", (MAX_ROUNDS, COLLAPSE_LENGTH), R)]
S3 = [("keep_reference", (), False), ("simplify", (EMPTY_ORIGIN, EMPTY_CELL), False), ("simplify_quadric", (SIMPLIFY_ORIGIN, QUADRIC_CELL), False), ("smooth", (SMOOTH_PASSES,), False),
      ("flip_edges", (MAX_ROUNDS,), False), ("fill_holes", (FILL_EDGES,), False), ("repair", (rc.SPLIT_PINCHES,), False),
      ("collapse_edges", (MAX_ROUNDS, COLLAPSE_LENGTH), False), ("split_edges", (MAX_ROUNDS, SPLIT_LENGTH), R), ("finalize", (), R)]
