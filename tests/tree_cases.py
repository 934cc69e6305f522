"""Clouds that drive the octree build where a uniform cloud never goes, and a brute-force statement of what a tree holds.

numpy only.  The builders are seeded and return SPLAT_DTYPE arrays (unit normals, quality in 0.5 .. 2); their arguments
are (n, levels, sub, size, offset, seed).  `entries` restates the per-splat part of the build (prepare / goodEntry, as
described beside splatEntries in mlsgpu_amd/csrc/octree.hip) in float32 numpy; `expected_walk` says which ids a walk from a
leaf must visit, in which order.  Neither sorts, scans or builds a command list, so they share nothing with the oracle's
tree but the arithmetic of one splat.
"""
import numpy as np

from oracle_binding import SPLAT_DTYPE

SORT_MAX_DIGIT_BITS = 10        # primitives.hpp: SortCaps<uint32_t>::MAX_DIGIT_BITS
FAR = 1.0e6                     # "far away": no entry, yet every coordinate converts to int without saturating
FACE_RADII = (0.05, 0.4, 1.0, 3.9, 7.9, 20.0, 70.0, 300.0)
FAR_RUN = 2048 + 100            # splats of a far run: at least one whole tile of 1024 wherever it begins


def shifts(levels, sub):
    """(minShift, maxShift) of a build."""
    max_shift = levels + sub - 1
    return min(sub, max_shift), max_shift


def max_size(levels, sub):
    return 1 << (levels + sub - 1)


def digit_bits(levels, sub):
    """(key bits, bits of the first pass's digit): the split treeBuildBatch makes."""
    lo, hi = shifts(levels, sub)
    key_bits = 3 * (hi - lo) + 1
    passes = (key_bits + SORT_MAX_DIGIT_BITS - 1) // SORT_MAX_DIGIT_BITS
    return key_bits, (key_bits + passes - 1) // passes


def morton(x, y, z):
    """Morton code, z major, of arrays (or ints) below 2^10."""
    x, y, z = (np.asarray(v, np.int64) for v in (x, y, z))
    code = np.zeros(np.broadcast(x, y, z).shape, np.int64)
    for b in range(10):
        code |= ((x >> b) & 1) << (3 * b) | ((y >> b) & 1) << (3 * b + 1) | ((z >> b) & 1) << (3 * b + 2)
    return code


def _finish(position, radius, rng):
    n = len(radius)
    s = np.zeros(n, SPLAT_DTYPE)
    s["position"] = np.asarray(position, np.float64).reshape(n, 3).astype(np.float32)
    s["radius"] = np.asarray(radius, np.float64).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm[(nrm * nrm).sum(axis=1) == 0] = 1.0
    s["normal"] = (nrm / np.sqrt((nrm * nrm).sum(axis=1))[:, None]).astype(np.float32)
    s["quality"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
    return s


def _inside_nodes(nodes, sub, offset, rng):
    """One splat strictly inside each of the finest nodes [n, 3], radius 0.4: floor(p -/+ r) stays in the node's cells and
    the neighbours are 0.45 away, so each makes the one entry of its own node."""
    cell = float(1 << sub)
    local = nodes.astype(np.float64) * cell + rng.uniform(0.45, cell - 0.45, nodes.shape)
    return _finish(local + np.asarray(offset, np.float64), np.full(len(nodes), 0.4), rng)


def _nodes_per_axis(size, sub):
    return (np.asarray(size, np.int64) + (1 << sub) - 1) >> sub


def corners(n, levels, sub, size, offset, seed):
    """Eight entries per splat: the centre is the corner that eight nodes of one level share, the radius just short of half
    a node (so that level is the splat's own)."""
    rng = np.random.default_rng(seed)
    lo, hi = shifts(levels, sub)
    size = np.asarray(size, np.int64)
    usable = [s for s in range(lo, min(lo + 2, hi) + 1) if (size.min() >> s) >= 2]
    assert usable, "the grid has no inner node corner at any level"
    s = rng.choice(usable, n)
    k = rng.integers(1, np.maximum(size[None, :] >> s[:, None], 2))     # 1 .. size / 2^s - 1
    centre = np.asarray(offset, np.int64) + (k << s[:, None])
    return _finish(centre, (1 << s) / 2.0 - 0.1, rng)


def one_node(n, levels, sub, size, offset, seed):
    """Every splat in ONE finest node: one entry each, one key."""
    rng = np.random.default_rng(seed)
    lo, _ = shifts(levels, sub)
    node = rng.integers(0, np.maximum(np.asarray(size, np.int64) >> lo, 1))
    return _inside_nodes(np.tile(node, (n, 1)), lo, offset, rng)


def one_low_digit(n, levels, sub, size, offset, seed):
    """One entry each, in finest nodes whose coordinates are multiples of 8: the low 9 bits of every key are zero, so the
    first pass sees one digit and the keys differ only above it."""
    rng = np.random.default_rng(seed)
    lo, _ = shifts(levels, sub)
    per_axis = (_nodes_per_axis(size, lo) - 1) // 8 + 1
    return _inside_nodes(8 * rng.integers(0, per_axis, (n, 3)), lo, offset, rng)


def one_high_digit(n, levels, sub, size, offset, seed):
    """One entry each, spread over the finest nodes of ONE aligned cube of 8 x 8 x 8: the keys agree above their low 9 bits.
    The first pass's digit is narrower than 9 bits where the key has more than one digit (8 of 16 or 22 bits), and the bits
    of the cube above it belong to the next digit: the cloud keeps to the nodes on which those are zero (8 x 8 x 4 of them
    for an 8-bit digit), so that every first-pass digit occurs and what lies above is ONE value."""
    rng = np.random.default_rng(seed)
    lo, _ = shifts(levels, sub)
    _, per_pass = digit_bits(levels, sub)
    per_axis = _nodes_per_axis(size, lo)
    cube = 8 * rng.integers(0, np.maximum(per_axis // 8, 1))
    g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    g = g[((cube + g) < per_axis).all(axis=1)]
    g = g[(morton(*g.T) >> per_pass) == 0]
    return _inside_nodes(cube + g[rng.integers(0, len(g), n)], lo, offset, rng)


def far_runs(n):
    """[begin, end) of the runs of `faces` that lie far from the grid."""
    if n < 5000:
        return []
    runs = [(n // 4, n // 4 + FAR_RUN)]
    if n >= 12000:
        runs.append((3 * n // 4 - FAR_RUN // 2, 3 * n // 4 + FAR_RUN // 2))
    return runs


def far_away(n, levels, sub, size, offset, seed):
    """No entry at all: every splat FAR from the grid, on either side of it along a random axis."""
    rng = np.random.default_rng(seed)
    local = rng.uniform(0.0, 1.0, (n, 3)) * np.asarray(size, np.float64)
    local[np.arange(n), rng.integers(0, 3, n)] += rng.choice([-FAR, FAR], n)
    radius = rng.choice(FACE_RADII, n) * (1 << sub) / 8.0
    return _finish(local + np.asarray(offset, np.float64), radius, rng)


def faces(n, levels, sub, size, offset, seed):
    """Splats of every size on, across and beyond every face of the grid: from far smaller than a cell to larger than the
    grid, 12 cells beyond it on all sides; from 5000 splats on, runs of FAR_RUN consecutive splats far away."""
    rng = np.random.default_rng(seed)
    size = np.asarray(size, np.float64)
    local = -12.0 + rng.uniform(0.0, 1.0, (n, 3)) * (size + 24.0)
    radius = rng.choice(FACE_RADII, n) * (1 << sub) / 8.0
    s = _finish(local + np.asarray(offset, np.float64), radius, rng)
    for k, (b, e) in enumerate(far_runs(n)):
        s[b:e] = far_away(e - b, levels, sub, size, offset, seed + 1000 + k)
    return s


def far_corner(n, levels, sub, size, offset, seed):
    """The corner of the grid farthest from its origin: the last 120 cells below `size` on every axis and 3 beyond, where
    the high bits of the keys are set."""
    rng = np.random.default_rng(seed)
    local = np.asarray(size, np.float64) - 120.0 + rng.uniform(0.0, 123.0, (n, 3))
    radius = rng.uniform(0.5, 6.0, n) * (1 << sub) / 8.0
    return _finish(local + np.asarray(offset, np.float64), radius, rng)


BUILDERS = dict(corners=corners, one_node=one_node, one_low_digit=one_low_digit, one_high_digit=one_high_digit, faces=faces,
                far_corner=far_corner, far_away=far_away)


def ragged_size(levels, sub, cap=None):
    """The largest grid of the pair (capped), two axes a few cells short of it."""
    m = max_size(levels, sub) if cap is None else min(max_size(levels, sub), cap)
    return (m, m - 5, m - 8) if m > 8 else (m, m, m)


# --------------------------------------------------------------------------------------------------------------------------
# the brute force


class Entries:
    """Every entry of a build, in (splat, slot) order: rows of (id, shift, node x, y, z)."""

    def __init__(self, rows, min_shift, max_shift):
        self.rows, self.min_shift, self.max_shift = rows, min_shift, max_shift
        self._by_node = None

    def __len__(self):
        return len(self.rows)

    def keys(self):
        """The sort key of every entry: Morton code + where the level's nodes begin (finest level first)."""
        begin = np.zeros(self.max_shift + 1, np.int64)
        pos = 0
        for s in range(self.min_shift, self.max_shift + 1):
            begin[s] = pos
            pos += 1 << (3 * (self.max_shift - s))
        r = self.rows
        return morton(r[:, 2], r[:, 3], r[:, 4]) + begin[r[:, 1]]

    def by_node(self):
        """(shift, x, y, z) -> ids, ascending."""
        if self._by_node is None:
            r = self.rows
            order = np.lexsort((r[:, 4], r[:, 3], r[:, 2], r[:, 1]))     # stable: ids keep their (ascending) order in a node
            s = r[order]
            cut = np.flatnonzero((s[1:, 1:] != s[:-1, 1:]).any(axis=1)) + 1
            self._by_node = dict((tuple(g[0, 1:].tolist()), g[:, 0]) for g in np.split(s, cut) if len(g))
        return self._by_node


def entries(splats, first, offset, sub, levels, num=None):
    """The entries of splats[first : first + num] (all behind `first` by default)."""
    f32 = np.float32
    num = len(splats) - first if num is None else num
    min_shift, max_shift = shifts(levels, sub)
    p = splats["position"][first:first + num].astype(f32)
    r = splats["radius"][first:first + num].astype(f32)
    off = np.asarray(offset, np.int64)
    # prepare: floor of p -/+ r, the level from the widest extent, clamped to the tree's
    lo = np.floor(p - r[:, None]).astype(np.int64)
    hi = np.floor(p + r[:, None]).astype(np.int64)
    big = (hi - lo).max(axis=1) if num else np.zeros(0, np.int64)
    shift = np.zeros(num, np.int64)
    wide = big > 1
    shift[wide] = np.floor(np.log2((big[wide] - 1).astype(np.float64))).astype(np.int64) + 1      # bit length of big - 1
    assert np.all((big[wide] - 1) >> shift[wide] == 0) and np.all((big[wide] - 1) >> (shift[wide] - 1) == 1)
    shift = np.clip(shift, min_shift, max_shift)
    ilo = np.maximum(lo - off, 0) >> shift[:, None]
    radius2 = (r * r) * f32(1.00001)
    bound = np.int64(1) << (max_shift - shift)
    ids = np.arange(first, first + num, dtype=np.int64)
    out = []
    for o in range(8):
        a = ilo + np.array([o & 1, (o >> 1) & 1, o >> 2], np.int64)
        blo = ((a << shift[:, None]) + off).astype(f32)
        bhi = (((a + 1) << shift[:, None]) + off).astype(f32)
        d = np.maximum(blo, np.minimum(bhi, p)) - p                      # nearest point of the box - p
        dist2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]  # float32, a sum of products
        assert dist2.dtype == f32 and radius2.dtype == f32
        good = (dist2 < radius2) & (a < bound[:, None]).all(axis=1)
        out.append(np.column_stack([ids, shift, a, np.full(num, o), good]))
    rows = np.stack(out, axis=1).reshape(8 * num, 7)                     # (splat, slot) order
    rows = rows[rows[:, 6] != 0][:, :5]
    return Entries(rows, min_shift, max_shift)


def expected_walk(ent, leaf):
    """The ids (an int64 array) a walk from the finest node `leaf` (x, y, z) visits: those of its own node, ascending, then
    those of every coarser node that contains it, finest to coarsest."""
    d = ent.by_node()
    x, y, z = (int(v) for v in leaf)
    none = np.zeros(0, np.int64)
    parts = [d.get((s, x >> (s - ent.min_shift), y >> (s - ent.min_shift), z >> (s - ent.min_shift)), none)
             for s in range(ent.min_shift, ent.max_shift + 1)]
    return np.concatenate(parts)


def leaf_key(leaf):
    return int(morton(*leaf))


def tile_counts(ent, first, num, tile=1024):
    """Entries per tile of `tile` consecutive splats."""
    return np.bincount((ent.rows[:, 0] - first) // tile, minlength=(num + tile - 1) // tile)
