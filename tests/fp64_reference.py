"""Plain float64 restatement of the MLS corner field and of marching tetrahedra, for the tests only.

Written from the mathematics of the method, independent of the oracle (oracle/mlsgpu_oracle.cpp) and of the library: no
octree, no lookup tables.  The oracle and the HIP kernels are bit-identical by construction; this module is what ties
both to the mathematics.

MLS (the algebraic-sphere / plane fit of the reference's processCorners), per grid corner c:
  every splat i with d_i = |p_i - c|^2 * (1/r_i^2) < 0.99 is a hit, with weight w_i = (1 - d_i)^4 * quality_i;
  fewer than 4 hits: NaN.  With local positions x_i = p_i - c and normals n_i the weighted sums
  W = sum w, Wp = sum w x, Wn = sum w n, Wpp = sum w |x|^2, Wpn = sum w x.n fit
    sphere: m = Wp / W, q = (Wpn - m.Wn) / (Wpp - m.Wp) (0 when |qDen| < 4 eps32 hits |Wpp| or q is not finite),
            a = q / 2, b = (Wn - q Wp) / W, c = (-a Wpp - b.Wp) / W; the projection of the corner is
            A = l b with l the root of (a |b|^2) l^2 + |b|^2 l + c = 0 chosen as in solve_quadratic, the value -b.A / |b|
    plane:  mean = Wp / W, normal = Wn / |Wn|, dist = -normal.mean, A = -dist normal, the value dist;
  the value is kept only if |A|^2 < 3 and qDen > boundary_factor * sum w |x - A|^2 (qDen of the plane: Wpp - mean.Wp).

Marching (Kuhn decomposition of every cell into six tetrahedra around its 0-7 diagonal; corner index bit 0 = x, bit 1 = y,
bit 2 = z), on a float32 field [z, y, x]: a corner is outside iff iso >= 0 (so -0.0 is outside); a cell is valid iff its
eight corners are finite.  The tetrahedra's edges are the lattice segments p -> p + d for the seven directions d in
{0,1}^3 \\ {0}; an edge carries a vertex iff a valid cell holds it and its ends differ in outside-ness; the vertex is at
p + t d with t = iso(p) / (iso(p) - iso(p + d)).

The mesh comparison (match_vertices, triangles_in_tetrahedra) is valid up to 8192 corners a side: a point's tolerance is
march_tol, MARCH_TOL scaled by the binade of its largest coordinate (unchanged below 128), and the matcher buckets the edge
points of each binade by their own tolerance and keys the buckets by per-axis ranks, which fit an int64 where three bucket
coordinates of 8192 / 2.2e-5 each would not.  What was measured at which coordinates stands above MARCH_TOL.
"""
import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)
F32_TINY = float(np.finfo(np.float32).tiny)
RADIUS_CUTOFF = float(np.float32(0.99))
HITS_CUTOFF = 4

# ---- tolerances, pinned from measurement --------------------------------------------------------------------------------
# MLS: |oracle - fp64| (cells) over the non-ambiguous corners of tests/test_fp64_oracle.py (sphere, uniform, shells, planes,
# negative-offset clouds; trees (6,3) (4,4) (3,5) (7,3); both shapes; boundary limits 0 .. 3; 317 k values): max 2.2e-5
# (boundary limit 3, where the fit is weakest), 99th percentile 3.7e-7 overall and at most 8.0e-7 in any one run.
# The oracle is bit-identical to the kernels, so this is the kernels' error too.  Pinned at about 3x.
MLS_MAX_ABS = 6e-5
MLS_P99_ABS = 2.5e-6
# marching: |float32 vertex - fp64 vertex| over every unflagged edge of the GENERATE_CASES, the torus and the special-value
# fields (coordinates below 83): max 5.4e-6 = half an ulp of a coordinate in [64, 128) plus the error of t.  Pinned at 2x.
# Half an ulp doubles with every binade (6.1e-5 in [1024, 2048), 2.4e-4 in [4096, 8192)), so above 128 the tolerance of a
# point is MARCH_TOL * 2^(e - 6) with e = floor(log2(its largest |coordinate|)): march_tol below.  It IS MARCH_TOL for every
# coordinate below 128 and keeps its ratio to half an ulp (2.88) above.  Measured on the thin grids of
# tests/test_marching_extents_oracle.py (noise with NaN holes and a smooth tube; no vertex missing or extra, every triangle in
# its tetrahedron, the float32 formula pinned), the oracle's worst error and its share of the bound:
#   2049 x 5 x 4, 5 x 2049 x 4, 5 x 4 x 2049: 6.11e-5 = 0.348 - 0.350 (93 723 vertices on the first)
#   4100 x 5 x 4: 2.41e-4 (noise), 2.43e-4 (tube) = 0.349        8189 x 4 x 4: 2.44e-4 = 0.349 (287 206 vertices)
# Binade by binade on the 8189-long grid: 3.8e-6 below 128, 3.1e-5 in [128, 1024), 6.1e-5, 1.22e-4 and 2.44e-4 in the three
# above, each 0.347 - 0.349 of its bound: the error is half an ulp of the coordinate plus the error of t everywhere, which is
# what the scaling assumes.  The kernels' output on the 2049-long grids gives the same figures (bit-equal to the oracle).
MARCH_TOL = 1.1e-5

# ambiguity bands (relative): where float32 rounding may legitimately take the other branch of a comparison
CUTOFF_BAND = 1e-5        # |d - 0.99| <= band * 0.99 for some splat
AA_BAND = 1e-3            # |aa - 3| <= band * 3
BOUNDARY_BAND = 1e-4      # |qDen - bf rhs| <= band * (Wpp + |bf| (Wpp + 2 |Wp.A| + W aa))
DISC_BAND = 1e-4          # |disc| <= band * (B^2 + 4 |A C|)
QDEN_BAND = 2.0           # |qDen| within [thr / band, thr * band] or below 64 eps32 Wpp (thr = 4 eps32 hits Wpp)


# ------------------------------------------------------------------------------------------------------------------------
# MLS
# ------------------------------------------------------------------------------------------------------------------------

def mls_sums_fp64(splats, corners, weight_power=4, chunk=128):
    """Weighted sums of every corner over ALL splats (brute force).  `splats` is the SPLAT_DTYPE array as the kernel reads it
    (radius slot = 1/r^2); `corners` [n, 3] are the corner positions in grid units."""
    pos = splats["position"].astype(np.float64)
    inv_r2 = splats["radius"].astype(np.float64)
    nrm = splats["normal"].astype(np.float64)
    qual = splats["quality"].astype(np.float64)
    corners = np.asarray(corners, np.float64).reshape(-1, 3)
    n = len(corners)
    out = dict(W=np.zeros(n), Wp=np.zeros((n, 3)), Wn=np.zeros((n, 3)), Wpp=np.zeros(n), Wpn=np.zeros(n),
               hits=np.zeros(n, np.int64), near_cutoff=np.zeros(n, bool))
    for lo in range(0, n, chunk):
        c = corners[lo:lo + chunk]
        x = pos[None, :, :] - c[:, None, :]                     # [k, s, 3]
        pp = np.einsum("ksa,ksa->ks", x, x)
        with np.errstate(invalid="ignore", over="ignore"):
            d = pp * inv_r2[None, :]
            hit = d < RADIUS_CUTOFF
            out["near_cutoff"][lo:lo + len(c)] = np.any(np.abs(d - RADIUS_CUTOFF) <= CUTOFF_BAND * RADIUS_CUTOFF, axis=1)
        ci, si = np.nonzero(hit)
        w = (1.0 - d[ci, si]) ** weight_power * qual[si]
        xs = x[ci, si]
        k = len(c)
        out["W"][lo:lo + k] = np.bincount(ci, w, k)
        for a in range(3):
            out["Wp"][lo:lo + k, a] = np.bincount(ci, w * xs[:, a], k)
            out["Wn"][lo:lo + k, a] = np.bincount(ci, w * nrm[si, a], k)
        out["Wpp"][lo:lo + k] = np.bincount(ci, w * pp[ci, si], k)
        out["Wpn"][lo:lo + k] = np.bincount(ci, w * np.einsum("ia,ia->i", xs, nrm[si]), k)
        out["hits"][lo:lo + k] = np.bincount(ci, None, k).astype(np.int64)
    return out


def _dot(a, b):
    return np.einsum("ia,ia->i", a, b)


def _solve_quadratic(a, b, c):
    """Root of a x^2 + b x + c (b >= 0): -2c / (b + sqrt(b^2 - 4ac)), else (b + sqrt(.)) / (-2a), else NaN."""
    with np.errstate(all="ignore"):
        bdet = b + np.sqrt(b * b - 4.0 * a * c)
        x = -2.0 * c / bdet
        x = np.where(np.isfinite(x), x, bdet / (-2.0 * a))
    return np.where(np.isfinite(x), x, np.nan)


def mls_finish_fp64(s, shape, boundary_factor):
    """(value, ambiguous) of every corner from the sums of mls_sums_fp64."""
    W, Wp, Wn, Wpp, Wpn, hits = s["W"], s["Wp"], s["Wn"], s["Wpp"], s["Wpn"], s["hits"]
    bf = float(boundary_factor)
    n = len(W)
    ok = hits >= HITS_CUTOFF
    amb = s["near_cutoff"].copy()
    with np.errstate(all="ignore"):
        m = Wp / W[:, None]
        if shape == 0:
            qnum = Wpn - _dot(m, Wn)
            qden = Wpp - _dot(m, Wp)
            q = qnum / qden
            thr = 4 * F32_EPS * hits * np.abs(Wpp)
            unstable = (np.abs(qden) < thr) | ~np.isfinite(q)
            q = np.where(unstable, 0.0, q)
            aq = np.abs(qden)
            amb |= ok & (((aq >= thr / QDEN_BAND) & (aq <= thr * QDEN_BAND)) | (aq < 64 * F32_EPS * np.abs(Wpp)))
            a = 0.5 * q
            b = (Wn - q[:, None] * Wp) / W[:, None]
            c = (-a * Wpp - _dot(b, Wp)) / W
            b2 = _dot(b, b)
            qa, qb, qc = a * b2, b2, c
            disc = qb * qb - 4.0 * qa * qc
            amb |= ok & (np.abs(disc) <= DISC_BAND * (qb * qb + 4.0 * np.abs(qa * qc)))
            lam = _solve_quadratic(qa, qb, qc)
            A = lam[:, None] * b
            value = -_dot(b, A) / np.sqrt(b2)
        else:
            normal = Wn / np.sqrt(_dot(Wn, Wn))[:, None]
            dist = -_dot(normal, m)
            A = normal * -dist[:, None]
            qden = Wpp - _dot(m, Wp)
            value = dist
        aa = _dot(A, A)
        rhs = Wpp - 2 * _dot(Wp, A) + W * aa
        keep = ok & (aa < 3.0) & (qden > bf * rhs)
        amb |= ok & (np.abs(aa - 3.0) <= AA_BAND * 3.0)
        scale = np.abs(Wpp) + abs(bf) * (np.abs(Wpp) + 2 * np.abs(_dot(Wp, A)) + np.abs(W) * aa)
        amb |= ok & (aa < 3.0) & (np.abs(qden - bf * rhs) <= BOUNDARY_BAND * scale)
    out = np.full(n, np.nan)
    out[keep] = value[keep]
    return out, amb


def mls_field_fp64(splats, corners, shape, boundary_factor):
    """(value [n], ambiguous [n]) of the MLS field at `corners`, in float64 (NaN where the kernel writes NaN)."""
    return mls_finish_fp64(mls_sums_fp64(splats, corners), shape, boundary_factor)


def boundary_factor_fp64(limit):
    """1 - gamma^2 with gamma = limit * sqrt(6) * 512 / (693 pi) (the reference's boundary scale)."""
    g = float(limit) * np.sqrt(6.0) * 512 / (693 * np.pi)
    return 1.0 - g * g


def compare_field(got, exp, amb):
    """Oracle / kernel float32 values against the fp64 values on the non-ambiguous corners.  Returns a dict: nan_mismatch
    (count of corners where exactly one side is NaN), err (abs errors where both are numbers), ambiguous share."""
    got = np.asarray(got, np.float64)
    sel = ~amb
    gn, en = np.isnan(got[sel]), np.isnan(exp[sel])
    both = ~gn & ~en
    return dict(nan_mismatch=int(np.count_nonzero(gn != en)), err=np.abs(got[sel][both] - exp[sel][both]),
                ambiguous=float(np.mean(amb)) if len(amb) else 0.0, values=int(np.count_nonzero(both)))


def field_ok(cmp, max_abs=MLS_MAX_ABS, p99_abs=MLS_P99_ABS):
    e = cmp["err"]
    return (cmp["nan_mismatch"] == 0 and (len(e) == 0 or (e.max() <= max_abs and np.percentile(e, 99) <= p99_abs)))


# ------------------------------------------------------------------------------------------------------------------------
# marching
# ------------------------------------------------------------------------------------------------------------------------

CORNERS = np.array([[(i >> a) & 1 for a in range(3)] for i in range(8)], np.int64)      # corner index -> (x, y, z)
# the six tetrahedra around the 0-7 diagonal: 0 -> 7 through one corner with one coordinate set, then one with two
TETRAHEDRA = [(0, 1 << a, (1 << a) | (1 << b), 7) for a in range(3) for b in range(3) if a != b]
DIRECTIONS = np.array([[(k >> a) & 1 for a in range(3)] for k in range(1, 8)], np.int64)


def _tet_edges():
    """(o0, direction index) of the 19 distinct edges of the six tetrahedra of one cell."""
    seen = set()
    for t in TETRAHEDRA:
        for i in range(4):
            for j in range(i + 1, 4):
                lo, hi = CORNERS[min(t[i], t[j])], CORNERS[max(t[i], t[j])]
                d = hi - lo
                assert d.min() >= 0
                seen.add((tuple(lo), int(d[0] + 2 * d[1] + 4 * d[2]) - 1))
    return sorted(seen)


TET_EDGES = _tet_edges()
assert len(TET_EDGES) == 19


def marching_fp64(field):
    """Expected mesh of a float32 field [z, y, x] (grid coordinates, no key offset).  Returns a dict:
    edges [e, 3] int64 (2 p + d of every edge that carries a vertex, sorted), pos [e, 3] float64, flagged [e] (float32's
    iso0 - iso1 or its reciprocal is not a finite normal number, so float32 cannot follow float64), pos_f32 [e, 3] (what
    IEEE float32 arithmetic gives: t = iso0 * (1 / (iso0 - iso1)), p + t d, denormals kept), triangles (count)."""
    f = np.asarray(field, np.float32)
    D, H, W = f.shape
    out_ = f >= 0
    fin = np.isfinite(f)
    cz, cy, cx = D - 1, H - 1, W - 1
    valid = np.ones((cz, cy, cx), bool)
    for o in CORNERS:
        valid &= fin[o[2]:o[2] + cz, o[1]:o[1] + cy, o[0]:o[0] + cx]
    has = np.zeros((7, D, H, W), bool)
    for o0, k in TET_EDGES:
        d = DIRECTIONS[k]
        o1 = np.array(o0) + d
        a = out_[o0[2]:o0[2] + cz, o0[1]:o0[1] + cy, o0[0]:o0[0] + cx]
        b = out_[o1[2]:o1[2] + cz, o1[1]:o1[1] + cy, o1[0]:o1[0] + cx]
        has[k, o0[2]:o0[2] + cz, o0[1]:o0[1] + cy, o0[0]:o0[0] + cx] |= valid & (a != b)
    ntri = 0
    for t in TETRAHEDRA:
        n = sum(out_[CORNERS[v][2]:CORNERS[v][2] + cz, CORNERS[v][1]:CORNERS[v][1] + cy,
                     CORNERS[v][0]:CORNERS[v][0] + cx].astype(np.int64) for v in t)
        ntri += int(np.count_nonzero(valid & ((n == 1) | (n == 3)))) + 2 * int(np.count_nonzero(valid & (n == 2)))
    ks, zs, ys, xs = np.nonzero(has)
    p0 = np.stack([xs, ys, zs], axis=1).astype(np.int64)
    d = DIRECTIONS[ks]
    p1 = p0 + d
    i0 = f[p0[:, 2], p0[:, 1], p0[:, 0]]
    i1 = f[p1[:, 2], p1[:, 1], p1[:, 0]]
    t = i0.astype(np.float64) / (i0.astype(np.float64) - i1.astype(np.float64))
    pos = p0 + t[:, None] * d
    with np.errstate(all="ignore"):
        diff = i0 - i1
        inv = np.float32(1.0) / diff
        t32 = i0 * inv
        pos32 = p0.astype(np.float32) + t32[:, None] * d.astype(np.float32)
    normal = lambda v: np.isfinite(v) & (np.abs(v) >= F32_TINY)   # noqa: E731
    flagged = ~(normal(diff) & normal(inv))
    edges = 2 * p0 + d
    order = np.lexsort((edges[:, 0], edges[:, 1], edges[:, 2]))
    return dict(edges=edges[order], pos=pos[order], flagged=flagged[order], pos_f32=pos32[order].astype(np.float32),
                iso=np.stack([i0, i1], 1)[order], triangles=ntri)


def weld(batches):
    """refdata.weld_batches with the duplicate check done on bit patterns (a NaN vertex equals itself).
    Returns (vertices [n, 3] float32, triangles [m, 3] int64)."""
    verts, tris, key_map = [], [], {}
    for b in batches:
        nv, ni = len(b["vertices"]), b["num_internal"]
        remap = np.zeros(nv, np.int64)
        remap[:ni] = len(verts) + np.arange(ni)             # internal vertices come first and are never shared
        verts.extend(b["vertices"][:ni])
        for i in range(ni, nv):
            k = int(b["keys"][i])
            if k in key_map:
                assert np.array_equal(verts[key_map[k]].view(np.uint32), b["vertices"][i].view(np.uint32))
                remap[i] = key_map[k]
                continue
            key_map[k] = len(verts)
            remap[i] = len(verts)
            verts.append(b["vertices"][i])
        if len(b["triangles"]):
            tris.append(remap[b["triangles"].astype(np.int64)])
    v = np.array(verts, np.float32).reshape(-1, 3)
    t = np.concatenate(tris) if tris else np.zeros((0, 3), np.int64)
    return v, t


def _canon_bits(v):
    """Rows of float32 bit patterns with every NaN made one pattern."""
    b = np.ascontiguousarray(v, np.float32).copy()
    b[np.isnan(b)] = np.float32(np.nan)
    return b.view(np.uint32)


def same_vertex_multiset(verts, expected_f32):
    """Is the multiset of mesh vertices bit-equal to the multiset `expected_f32` (NaN == NaN)?"""
    a, b = _canon_bits(verts), _canon_bits(expected_f32)
    if a.shape != b.shape:
        return False
    a = a[np.lexsort(a.T[::-1])] if len(a) else a
    b = b[np.lexsort(b.T[::-1])] if len(b) else b
    return bool(np.array_equal(a, b))


def march_tol(pos, tol=MARCH_TOL):
    """Tolerance of every position [n, 3]: tol * max(1, 2^(e - 6)) with e = floor(log2(largest |coordinate|)), i.e. `tol`
    itself below 128 and the same multiple of half a float32 ulp in every binade above (non-finite rows: tol)."""
    p = np.abs(np.asarray(pos, np.float64).reshape(-1, 3))
    big = np.where(np.all(np.isfinite(p), axis=1), p.max(axis=1, initial=0.0), 0.0)
    _, e = np.frexp(big)                                  # big = m 2^e with m in [0.5, 1): floor(log2 big) = e - 1
    return tol * np.ldexp(1.0, np.maximum(e - 7, 0))


def _bucket_candidates(v, vi_all, P, pe, h):
    """(vertex, edge) index pairs whose buckets of width h touch (the 27 neighbours): vertices v[vi_all], edge points P[pe].
    A bucket's key is built from the per-axis RANKS of the edge points' bucket coordinates (at most len(pe) distinct values
    an axis), not from the coordinates themselves: three coordinates of 8192 / h each do not fit one int64, their ranks do."""
    bp = np.floor(P[pe] / h).astype(np.int64)
    axes = [np.unique(bp[:, a]) for a in range(3)]
    n = [len(u) for u in axes]
    assert n[0] * n[1] * n[2] < 2 ** 63

    def rank(a, b):
        """Rank of the bucket coordinates b on axis a, and whether each occurs among the edge points at all."""
        r = np.minimum(np.searchsorted(axes[a], b), n[a] - 1)
        return r, axes[a][r] == b
    pr = [rank(a, bp[:, a])[0] for a in range(3)]
    pc = (pr[2] * n[1] + pr[1]) * n[0] + pr[0]
    order = np.argsort(pc, kind="stable")
    pcs = pc[order]
    bv = np.floor(v[vi_all] / h).astype(np.int64)
    vr = [[rank(a, bv[:, a] + o) for o in (-1, 0, 1)] for a in range(3)]
    cand_v, cand_e = [], []
    for off in np.array(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij")).reshape(3, -1).T:
        (rx, kx), (ry, ky), (rz, kz) = (vr[a][off[a] + 1] for a in range(3))
        at = np.nonzero(kx & ky & kz)[0]
        if len(at) == 0:
            continue
        c = (rz[at] * n[1] + ry[at]) * n[0] + rx[at]
        a = np.searchsorted(pcs, c, "left")
        cnt = np.searchsorted(pcs, c, "right") - a
        if cnt.sum() == 0:
            continue
        rep = np.repeat(at, cnt)
        idx = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(a, cnt)
        cand_v.append(vi_all[rep])
        cand_e.append(pe[order[idx]])
    return cand_v, cand_e


def match_vertices(verts, ref, tol=MARCH_TOL):
    """Match mesh vertices to the expected unflagged edge points (nearest first, each used once, within the edge point's
    march_tol).  Returns dict(missing, extra, max_err, max_err_over_tol, vertex_edge): missing = unflagged edges no vertex
    matched; extra = vertices left over beyond one per flagged edge (negative: too few); max_err_over_tol = the largest
    distance of a matched pair as a share of that edge point's tolerance; vertex_edge[i] = edge index of vertex i or -1."""
    v = np.asarray(verts, np.float64)
    sel = np.nonzero(~ref["flagged"])[0]
    P = ref["pos"][sel]
    vertex_edge = np.full(len(v), -1, np.int64)
    if len(P) == 0 or len(v) == 0:
        return dict(missing=len(P), extra=len(v) - int(ref["flagged"].sum()), max_err=0.0, max_err_over_tol=0.0,
                    vertex_edge=vertex_edge)
    ptol = march_tol(P, tol)
    vi_all = np.nonzero(np.all(np.isfinite(v), axis=1))[0]
    vtol = march_tol(v[vi_all], tol)
    cand_v, cand_e = [], []
    for t in np.unique(ptol):                       # the edge points of one binade: buckets as wide as twice their tolerance
        # (a vertex within t of such a point lies in its binade or, across a power of two, in the one next to it)
        near = vi_all[(vtol >= 0.5 * t) & (vtol <= 2.0 * t)]
        cv, ce = _bucket_candidates(v, near, P, np.nonzero(ptol == t)[0], 2.0 * t)
        cand_v += cv
        cand_e += ce
    used_e = np.zeros(len(P), bool)
    max_err = max_ratio = 0.0
    if cand_v:
        cv, ce = np.concatenate(cand_v), np.concatenate(cand_e)
        dist = np.sqrt(((v[cv] - P[ce]) ** 2).sum(axis=1))
        keep = dist <= ptol[ce]
        cv, ce, dist = cv[keep], ce[keep], dist[keep]
        # a pair whose vertex and edge point occur in no other pair is taken whatever the order; the greedy pass is for the rest
        lone = (np.bincount(cv, minlength=len(v))[cv] == 1) & (np.bincount(ce, minlength=len(P))[ce] == 1)
        vertex_edge[cv[lone]] = sel[ce[lone]]
        used_e[ce[lone]] = True
        if lone.any():
            max_err = float(dist[lone].max())
            max_ratio = float((dist[lone] / ptol[ce[lone]]).max())
        cv, ce, dist = cv[~lone], ce[~lone], dist[~lone]
        o = np.argsort(dist, kind="stable")
        for i in o:
            if vertex_edge[cv[i]] < 0 and not used_e[ce[i]]:
                vertex_edge[cv[i]] = sel[ce[i]]
                used_e[ce[i]] = True
                max_err = max(max_err, float(dist[i]))
                max_ratio = max(max_ratio, float(dist[i] / ptol[ce[i]]))
    missing = int(np.count_nonzero(~used_e))
    extra = int(np.count_nonzero(vertex_edge < 0)) - int(ref["flagged"].sum())
    return dict(missing=missing, extra=extra, max_err=max_err, max_err_over_tol=max_ratio, vertex_edge=vertex_edge)


def triangles_in_tetrahedra(verts, tris, tol=MARCH_TOL):
    """Number of triangles whose three vertices do NOT all lie in one Kuhn tetrahedron of one cell (0 = all fine), every
    vertex within its own march_tol.  Triangles with a non-finite vertex are skipped."""
    v = np.asarray(verts, np.float64)[np.asarray(tris, np.int64)]       # [m, 3 vertices, 3 axes]
    v = v[np.all(np.isfinite(v), axis=(1, 2))]
    if len(v) == 0:
        return 0
    vt = march_tol(v.reshape(-1, 3), tol).reshape(-1, 3)                 # [m, 3 vertices]
    cen = v.mean(axis=1)
    cell = np.floor(cen)
    loc = v - cell[:, None, :]                                           # local coordinates of the three vertices
    lc = cen - cell
    srt = np.argsort(-lc, axis=1, kind="stable")                         # the tetrahedron: u_srt0 >= u_srt1 >= u_srt2
    u = np.take_along_axis(loc, np.repeat(srt[:, None, :], 3, axis=1), axis=2)
    ok = np.all((loc >= -vt[:, :, None]) & (loc <= 1 + vt[:, :, None]), axis=(1, 2))
    ok &= np.all(u[:, :, 0] - u[:, :, 1] >= -vt, axis=1) & np.all(u[:, :, 1] - u[:, :, 2] >= -vt, axis=1)
    return int(np.count_nonzero(~ok))


def signed_volume(verts, tris):
    """Volume enclosed by the triangles with finite vertices (positive: counter-clockwise seen from outside)."""
    v = np.asarray(verts, np.float64)
    t = np.asarray(tris, np.int64)
    t = t[np.all(np.isfinite(v[t]), axis=(1, 2))]
    if len(t) == 0:
        return 0.0
    c = v[t.ravel()].mean(axis=0)
    a, b, d = (v[t[:, k]] - c for k in range(3))
    return float(np.einsum("ia,ia->", a, np.cross(b, d)) / 6.0)


def euler_characteristic(num_vertices, tris):
    t = np.asarray(tris, np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    return int(num_vertices - len(np.unique(e, axis=0)) + len(t))


def compare_mesh(batches, ref, tol=MARCH_TOL):
    """Everything the tests assert about a mesh against marching_fp64's `ref`, in one dict."""
    v, t = weld(batches)
    m = match_vertices(v, ref, tol)
    return dict(vertices=len(v), triangles=len(t), missing=m["missing"], extra=m["extra"], max_err=m["max_err"],
                max_err_over_tol=m["max_err_over_tol"],
                triangles_match=len(t) == ref["triangles"], off_tetrahedron=triangles_in_tetrahedra(v, t, tol),
                volume=signed_volume(v, t) if len(t) else 0.0, euler=euler_characteristic(len(v), t) if len(t) else 0,
                f32_pinned=same_vertex_multiset(v, ref["pos_f32"]), welded=(v, t))


def mesh_ok(c):
    return c["missing"] == 0 and c["extra"] == 0 and c["triangles_match"] and c["off_tetrahedron"] == 0
