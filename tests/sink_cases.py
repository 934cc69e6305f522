"""Inputs for the mesh sinks (device: csrc/mesher.hip, host: csrc/host_mesher.hip) that leave the smallest operating point:
thousands of components, several 4 096-element waves and sort tiles, hundreds of blocks, keys shared by eight blocks in
several chunks, empty blocks of every kind, and vertex numberings that make long union-find chains.

Pure numpy, seeded.  Every welded vertex has a unique position with small integer coordinates (sheets and ribbons lie at
z < 5, islands at z = 100.., the extra vertices of with_empties at z = 200..), so mesher_oracle.isomorphic applies.
A mesh is the dict mesher_cases.mesh() makes: chunk, vertices (internal first), num_internal, keys, triangles."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import mesher_oracle as mo  # noqa: E402

E = np.uint64(1) << np.uint64(63)


def sheet_key(x, y):
    return E | (np.asarray(y, np.uint64) << np.uint64(21)) | np.asarray(x, np.uint64)


def sheet_position(x, y):
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    return np.stack([x, y, (y * 7 + x * 3) % 5], axis=-1).astype(np.float32)


def random_chunks(seed, chunks):
    """The default chunk_of: every block draws its chunk at random, so the chunks arrive interleaved."""
    def chunk_of(tile_x, tile_y, half):
        return np.random.default_rng([seed, 0xC4]).integers(0, chunks, len(tile_x))
    return chunk_of


def tiled_sheet(seed, width, height, tile, gap, split, chunks, chunk_of=None, corners=()):
    """A width x height sheet of quads (vertices (x, y), 0 <= x <= width, 0 <= y <= height) cut into tile x tile tiles.
    A share `gap` of the quads is missing; a share `split` of the tiles deals its triangles to two blocks.  A vertex is
    external if it lies on a tile border (x or y a multiple of `tile`) or if both halves of its tile use it; its key is
    1<<63 | y<<21 | x.  Blocks arrive tile by tile in row-major order, the two halves of a tile one after the other, and
    get their chunk from chunk_of(tile_x, tile_y, half) (arrays, one entry per block; default random_chunks(seed, chunks)).
    corners: tile corners (x, y), both multiples of `tile` and inside the sheet: the four quads around them are kept, their
    four tiles split, their diagonals run through the corner and their two triangles go to different halves, so that
    all eight blocks use the corner vertex."""
    rng = np.random.default_rng(seed)
    tiles_x = -(-width // tile)
    present = rng.random((height, width)) >= gap
    diagonal = rng.integers(0, 2, (height, width))           # 0: a-c, 1: b-d   (a = (x, y), b = (x+1, y), c = (x+1, y+1), d = (x, y+1))
    is_split = rng.random((-(-height // tile), tiles_x)) < split
    half = rng.integers(0, 2, (height, width, 2))            # the half of a split tile that takes the quad's triangle 0 / 1
    for cx, cy in corners:
        assert cx % tile == 0 and cy % tile == 0 and 0 < cx < width and 0 < cy < height
        for qx, qy, diag in ((cx, cy, 0), (cx - 1, cy, 1), (cx - 1, cy - 1, 0), (cx, cy - 1, 1)):
            present[qy, qx] = True
            diagonal[qy, qx] = diag                          # both triangles of the quad hold the corner
            half[qy, qx] = (0, 1)
            is_split[qy // tile, qx // tile] = True
    qy, qx = np.nonzero(present)
    stride = width + 1
    a, b, c, d = qy * stride + qx, qy * stride + qx + 1, (qy + 1) * stride + qx + 1, (qy + 1) * stride + qx
    diag = diagonal[qy, qx][:, None] == 0
    tri = np.stack([np.where(diag, np.stack([a, b, c], 1), np.stack([a, b, d], 1)),
                    np.where(diag, np.stack([a, c, d], 1), np.stack([b, c, d], 1))], axis=1).reshape(-1, 3)
    tile_of = np.repeat((qy // tile) * tiles_x + qx // tile, 2)
    tri_half = np.where(is_split.reshape(-1)[tile_of], half[qy, qx].reshape(-1), 0)
    block_code = tile_of * 2 + tri_half
    by_block = np.argsort(block_code, kind="stable")
    tri, block_code = tri[by_block], block_code[by_block]
    codes, block_of_tri = np.unique(block_code, return_inverse=True)        # blocks that have triangles, in arrival order
    nb = len(codes)
    # the vertices every block uses: (block, vertex) pairs
    nvid = stride * (height + 1)
    pair = np.unique((block_of_tri[:, None] * nvid + tri).reshape(-1))
    p_block, p_vid = pair // nvid, pair % nvid
    p_x, p_y = p_vid % stride, p_vid // stride
    partner = np.searchsorted(codes, codes[p_block] ^ 1)                    # the other half of the tile, if it is a block
    partner_ok = (partner < nb) & (codes[np.minimum(partner, nb - 1)] == (codes[p_block] ^ 1))
    external = (p_x % tile == 0) | (p_y % tile == 0) | (partner_ok & np.isin(partner * nvid + p_vid, pair))
    local_order = np.lexsort((p_vid, external, p_block))                    # per block: internal first, then by vertex id
    pair, p_block, p_x, p_y, external = pair[local_order], p_block[local_order], p_x[local_order], p_y[local_order], external[local_order]
    v_first = np.searchsorted(p_block, np.arange(nb + 1))
    local = np.arange(len(pair)) - v_first[p_block]
    sorter = np.argsort(pair)
    tri_local = local[sorter[np.searchsorted(pair, block_of_tri[:, None] * nvid + tri, sorter=sorter)]].astype(np.uint32)
    t_first = np.searchsorted(block_of_tri, np.arange(nb + 1))
    positions, keys = sheet_position(p_x, p_y), sheet_key(p_x, p_y)
    tile_x, tile_y = (codes // 2) % tiles_x, (codes // 2) // tiles_x
    chunk = np.asarray((chunk_of or random_chunks(seed, chunks))(tile_x, tile_y, codes % 2))
    meshes = []
    for k in range(nb):
        v0, v1 = v_first[k], v_first[k + 1]
        ext = external[v0:v1]
        meshes.append(dict(chunk=int(chunk[k]), vertices=positions[v0:v1], num_internal=int(len(ext) - ext.sum()),
                           keys=keys[v0:v1][ext], triangles=tri_local[t_first[k]:t_first[k + 1]]))
    return meshes


def with_islands(meshes, count):
    """One more block (in the last block's chunk) of `count` disjoint triangles, all vertices internal: `count` components."""
    i = np.arange(3 * count)
    vertices = np.stack([i % 1024, i // 1024, np.full(len(i), 100)], axis=-1).astype(np.float32)
    return meshes + [dict(chunk=meshes[-1]["chunk"], vertices=vertices, num_internal=len(vertices),
                          keys=np.zeros(0, np.uint64), triangles=i.reshape(-1, 3).astype(np.uint32))]


def block_kind(mesh):
    if len(mesh["vertices"]) == 0:
        return "no_vertices"
    if len(mesh["triangles"]) == 0:
        return "no_triangles"
    if mesh["num_internal"] == len(mesh["vertices"]):
        return "no_external"
    return "regular"


EMPTY_KINDS = ("no_vertices", "no_triangles", "no_external")


def with_empties(meshes):
    """`meshes` (regular blocks: triangles and external vertices) with blocks of the three other kinds at the front, in the
    middle and at the end: no vertices at all; vertices and keys but no triangles (keys of the neighbouring block, two keys
    nobody else has, one internal vertex); triangles but no external vertex (one quad).  They take the chunk of a block that
    is NOT their neighbour, so that an empty block may be a chunk's first arrival.  Three chunks are new: `extra` (first
    seen in the middle) has only blocks without triangles, `extra + 1` has one block of one 3-vertex triangle -- any prune
    threshold above 3 vertices removes that chunk -- and `extra + 2` (the last arrival) has only blocks without vertices,
    so that the chunk table ends past the last vertex and the last triangle."""
    assert all(block_kind(m) == "regular" for m in meshes) and len(meshes) >= 4
    extra = max(m["chunk"] for m in meshes) + 1
    counter = [0]

    def fresh(n, z):                                           # positions no other vertex has
        first = counter[0]
        counter[0] += n
        i = np.arange(first, first + n)
        return np.stack([i % 512, i // 512, np.full(n, z)], axis=-1).astype(np.float32), i

    def no_vertices(chunk):
        return dict(chunk=chunk, vertices=np.zeros((0, 3), np.float32), num_internal=0, keys=np.zeros(0, np.uint64),
                    triangles=np.zeros((0, 3), np.uint32))

    def no_triangles(chunk, neighbour):
        ni = neighbour["num_internal"]
        take = slice(ni, ni + min(5, len(neighbour["keys"])))
        own, i = fresh(2, 201)                                  # keys nobody else has, beyond every sheet's x range
        inner, _ = fresh(1, 200)
        return dict(chunk=chunk, vertices=np.concatenate([inner, neighbour["vertices"][take], own]), num_internal=1,
                    keys=np.concatenate([neighbour["keys"][:take.stop - ni], sheet_key(i + (1 << 20), np.zeros_like(i))]),
                    triangles=np.zeros((0, 3), np.uint32))

    def no_external(chunk):
        v, _ = fresh(4, 202)
        return dict(chunk=chunk, vertices=v, num_internal=4, keys=np.zeros(0, np.uint64),
                    triangles=np.array([[0, 1, 2], [0, 2, 3]], np.uint32))

    def trio(chunk, neighbour):
        return [no_vertices(chunk), no_triangles(chunk, neighbour), no_external(chunk)]

    mid = len(meshes) // 2
    island, _ = fresh(3, 203)
    out = trio(meshes[-1]["chunk"], meshes[0]) + meshes[:mid]
    out += trio(meshes[0]["chunk"], meshes[mid]) + [no_vertices(extra), no_triangles(extra, meshes[mid - 1])]
    out += meshes[mid:] + [no_triangles(extra, meshes[-1])]
    out += [dict(chunk=extra + 1, vertices=island, num_internal=3, keys=np.zeros(0, np.uint64),
                 triangles=np.array([[0, 1, 2]], np.uint32))]
    out += trio(meshes[mid]["chunk"], meshes[-1]) + [no_vertices(extra + 2), no_vertices(extra + 2)]
    return out


NUMBERINGS = ("ascending", "descending", "zigzag", "shuffled")


def ribbon(columns, numbering, seed=5):
    """A strip of 2 x columns vertices in one block, all internal, one component.  Along the strip (column by column) the
    vertex ids ascend, descend, alternate from both ends or are shuffled: the union-find hooks larger ids under smaller
    ones, so the numbering decides how long the parent chains get."""
    n = 2 * columns
    s = np.arange(n)                                            # position along the strip: column s // 2, row s % 2
    if numbering == "ascending":
        vid = s
    elif numbering == "descending":
        vid = n - 1 - s
    elif numbering == "zigzag":
        vid = np.where(s % 2 == 0, s // 2, n - 1 - s // 2)
    else:
        assert numbering == "shuffled"
        vid = np.random.default_rng(seed).permutation(n)
    vertices = np.zeros((n, 3), np.float32)
    vertices[vid] = np.stack([s // 2, s % 2, np.zeros(n)], axis=-1)
    q = 2 * np.arange(columns - 1)                             # quad between columns i and i + 1: strip positions q .. q + 3
    tri = np.stack([np.stack([q, q + 2, q + 3], 1), np.stack([q, q + 3, q + 1], 1)], axis=1).reshape(-1, 3)
    return [dict(chunk=0, vertices=vertices, num_internal=n, keys=np.zeros(0, np.uint64), triangles=vid[tri].astype(np.uint32))]


RIBBON_COLUMNS = 16384


def pick_corners(seed, width, height, tile, count):
    """`count` tile corners inside the sheet, seeded, no two the same."""
    rng = np.random.default_rng([seed, 0xC0])
    nx, ny = -(-width // tile) - 1, -(-height // tile) - 1     # interior corners per row / column
    pick = rng.choice(nx * ny, count, replace=False)
    return [(int(p % nx + 1) * tile, int(p // nx + 1) * tile) for p in pick]


def corner_chunks(seed, chunks, tile, corner):
    """random_chunks, but the four tiles around `corner` take chunk 0 with both halves."""
    def chunk_of(tile_x, tile_y, half):
        chunk = random_chunks(seed, chunks)(tile_x, tile_y, half)
        around = (np.abs(2 * tile_x + 1 - 2 * (corner[0] // tile)) == 1) & (np.abs(2 * tile_y + 1 - 2 * (corner[1] // tile)) == 1)
        return np.where(around, 0, chunk)
    return chunk_of


def components(meshes):
    return mo.mesh_sink(meshes)[1]["components"]


def _roots(target):
    base = tiled_sheet(12, 128, 128, 16, 0.72, 0.7, 3)
    return with_islands(base, target - components(base))


CORNERS = pick_corners(3, 96, 96, 8, 20)
CASES = {       # 0.2 s for all of them
    "many_components": tiled_sheet(11, 256, 256, 16, 0.72, 0.7, 5),
    "roots_2048": _roots(2048),
    "roots_2049": _roots(2049),
    "corners": tiled_sheet(3, 96, 96, 8, 0.6, 0.5, 4, chunk_of=corner_chunks(3, 4, 8, CORNERS[0]), corners=CORNERS),
    "many_blocks": tiled_sheet(14, 192, 192, 6, 0.72, 0.3, 7),
    "empties": with_empties(tiled_sheet(15, 64, 64, 8, 0.5, 0.5, 3)),
}
for _numbering in NUMBERINGS:
    CASES["ribbon_" + _numbering] = ribbon(RIBBON_COLUMNS, _numbering)
TILED = ("many_components", "roots_2048", "roots_2049", "corners", "many_blocks")
_EXPECTED = {}
STAT_NAMES = ("total_vertices", "threshold", "components", "kept_components", "kept_vertices", "kept_triangles")


def expected_boundary(name):
    if name not in _EXPECTED:
        _EXPECTED[name] = mo.expected_boundary(CASES[name])
    return _EXPECTED[name]


def prune_of(name):
    """(fraction, threshold in vertices) of the case's non-zero prune run.  With more than one component size the threshold
    lies halfway between the smallest and the largest component, so that some but not all components stay; a ribbon is one
    component, and its threshold is its whole vertex count: the `>=` of the prune rule at equality, everything stays."""
    sizes = expected_boundary(name)[2].astype(np.int64)
    total = int(sizes.sum())
    if name == "empties":
        fraction = 0.01                                         # the issue's: removes the island chunk
    elif sizes.min() == sizes.max():
        fraction = 1.0
    else:
        fraction = ((int(sizes.min()) + int(sizes.max()) + 1) // 2 + 0.5) / total
    return fraction, int(np.uint64(total * fraction))
