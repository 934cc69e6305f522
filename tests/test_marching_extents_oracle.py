"""The marching extent cases (tests/marching_extent_cases.py) on the CPU: the oracle against float64 on grids of up to 8189
corners a side, and the conditions under which a case covers the kernel path it was chosen for.

test_gpu_marching_extents.py holds the kernels to the oracle on these cases bit for bit; this file holds the oracle to the
mathematics at coordinates up to 8188 (fp64_reference.march_tol scales the tolerance with the coordinate's binade, and the
matcher keys its buckets by ranks, so the checker is valid there), and asserts -- not merely reports -- that every lattice
width occurs, that the noise field is dense enough for the rows route and the tube sparse enough for the cells route, that
two slices of mesh memory do overflow, and that every case has triangles."""
import numpy as np
import pytest

import fp64_reference as fr
import marching_extent_cases as mx


# ---- the widened checker -------------------------------------------------------------------------------------------------

def test_tolerance_scales_with_the_binade():
    """march_tol is MARCH_TOL for every coordinate below 128 (nothing existing weakens) and keeps its ratio to half a
    float32 ulp above: 2^(e - 6) times it in [2^e, 2^(e + 1))."""
    assert fr.MARCH_TOL == 1.1e-5
    rng = np.random.default_rng(5)
    low = np.concatenate([rng.uniform(-128, 128, (4000, 3)), [[0, 0, 0], [127.999999, 0, 0], [0, -127.999999, 3], [1e-30, 0, 0],
                                                             [np.nextafter(128.0, 0), 5, 5]]])
    assert np.all(fr.march_tol(low) == fr.MARCH_TOL)
    for e in range(7, 14):
        lo, hi = 2.0 ** e, np.nextafter(2.0 ** (e + 1), 0)
        p = np.array([[lo, 1, 2], [3, -hi, 4], [5, 6, 0.5 * (lo + hi)], [lo, hi, lo]])
        assert np.all(fr.march_tol(p) == fr.MARCH_TOL * 2.0 ** (e - 6)), e
        half_ulp = 0.5 * float(np.spacing(np.float32(lo)))
        assert fr.march_tol(p)[0] / half_ulp == fr.MARCH_TOL / (0.5 * float(np.spacing(np.float32(64.0))))
    assert np.all(fr.march_tol(np.array([[np.nan, 1, 2], [np.inf, 0, 0]])) == fr.MARCH_TOL)
    assert fr.march_tol(np.array([[4000.0, 0, 0]]), 1e-3)[0] == 1e-3 * 32


def test_matcher_at_large_coordinates():
    """The matcher on points spread over 8192^3 (where a product of bucket spans would pass 2^63): every point matched to
    itself moved by a third of its tolerance, and one moved by twice its tolerance is reported missing and extra."""
    rng = np.random.default_rng(9)
    P = np.concatenate([rng.uniform(0, 8190, (5000, 3)), rng.uniform(0, 100, (2000, 3)), [[8188.5, 8188.0, 8188.0], [0.5, 0, 0]]])
    ref = dict(pos=P, flagged=np.zeros(len(P), bool))
    tol = fr.march_tol(P)
    d = rng.normal(size=P.shape)
    d /= np.linalg.norm(d, axis=1)[:, None]
    perm = rng.permutation(len(P))
    v = (P + d * tol[:, None] / 3)[perm]
    m = fr.match_vertices(v, ref)
    assert m["missing"] == 0 and m["extra"] == 0
    assert np.array_equal(m["vertex_edge"], perm)
    assert 0.33 < m["max_err_over_tol"] < 0.34
    far = int(np.argmax(P[perm][:, 0]))                     # a vertex at x > 8000: tolerance 64 MARCH_TOL
    assert fr.march_tol(P[perm][far:far + 1])[0] == 64 * fr.MARCH_TOL
    v[far] = P[perm][far] + d[perm][far] * 2 * tol[perm][far]
    m = fr.match_vertices(v, ref)
    assert m["missing"] == 1 and m["extra"] == 1 and m["vertex_edge"][far] == -1
    # near the origin the tolerance is still MARCH_TOL itself: what a far vertex may be off by is an error there
    near = int(np.argmin(np.abs(P[perm]).max(axis=1)))
    v = (P + d * tol[:, None] / 3)[perm]
    v[near] = P[perm][near] + d[perm][near] * 2 * fr.MARCH_TOL
    m = fr.match_vertices(v, ref)
    assert m["missing"] == 1 and m["extra"] == 1 and m["vertex_edge"][near] == -1


# ---- the oracle against float64 --------------------------------------------------------------------------------------------

def check_wide_mesh(batches, ref, name):
    """check_mesh of test_fp64_oracle.py with the error held to every vertex's own bound; prints the worst error over it."""
    c = fr.compare_mesh(batches, ref)
    print("%s: %d vertices, %d triangles, max_err %.3g = %.3f of its bound" % (name, c["vertices"], c["triangles"], c["max_err"],
                                                                               c["max_err_over_tol"]))
    assert c["missing"] == 0 and c["extra"] == 0, (name, c["missing"], c["extra"])
    assert c["triangles_match"], (name, c["triangles"], ref["triangles"])
    assert c["off_tetrahedron"] == 0, name
    assert c["max_err_over_tol"] <= 1.0, (name, c["max_err_over_tol"])
    assert c["f32_pinned"], name
    return c


@pytest.mark.parametrize("size", mx.THIN_SIZES, ids=lambda s: "%dx%dx%d" % tuple(s))
@pytest.mark.parametrize("field", ["noise", "tube"])
def test_oracle_vs_fp64_on_thin_grids(field, size):
    """Noise (NaN holes, every code) and a smooth tube on grids 2049 to 8189 corners long in x, y or z and 4 or 5 across:
    no vertex missing or extra, the triangle count, every triangle inside one tetrahedron, the float32 formula pinned."""
    case = mx.thin_case(field, size)
    batches, st = mx.oracle_run(case, "ample", (0, 0, 0))
    ref = fr.marching_fp64(mx.field_array(case.fn, case.size))
    assert len(ref["edges"]) > 10 * max(size) and ref["triangles"] > 10 * max(size)
    assert not ref["flagged"].any()
    c = check_wide_mesh(batches, ref, case.name)
    assert st["welded"] == c["vertices"] and st["indices"] == 3 * c["triangles"]
    assert float(np.abs(c["welded"][0]).max()) > max(size) - 2          # the mesh does reach the far end


def test_sensitivity_at_large_coordinates():
    """One vertex of the 2049-wide mesh moved by an ulp and a half of its coordinate (1.8e-4 at x in [1024, 2048), beyond its
    bound of 1.76e-4): missing and extra, as on the small grids."""
    case = mx.thin_case("noise", (2049, 5, 4))
    batches, _ = mx.oracle_run(case, "ample", (0, 0, 0))
    ref = fr.marching_fp64(mx.field_array(case.fn, case.size))
    moved = [dict(b) for b in batches]
    v = moved[0]["vertices"].copy()
    i = int(np.argmax(v[:, 0] * (v[:, 0] < 2040)))
    assert 1024 < v[i, 0] < 2048
    v[i, 1] += np.float32(1.5 * 2.0 ** -13)
    moved[0]["vertices"] = v
    c = fr.compare_mesh(moved, ref)
    assert c["missing"] == 1 and c["extra"] == 1 and not fr.mesh_ok(c)


# ---- the conditions the GPU tests rely on ----------------------------------------------------------------------------------

def test_every_lattice_width_occurs():
    nws = {mx.lattice_words(w) for w in mx.WIDTHS}
    assert set(mx.NW_REQUIRED) <= nws, sorted(set(mx.NW_REQUIRED) - nws)
    assert max(mx.WIDTHS) + 3 == 8192                       # the widest case is constructed with the API's limit
    assert {w - 1 for w in mx.WIDTHS} >= {128, 129, 192, 193, 384, 385}
    assert set(mx.REGIME_WIDTHS) <= set(mx.WIDTHS)
    assert sorted(mx.lattice_words(w) > 64 for w in mx.REGIME_WIDTHS) == [False] * 4 + [True]


def check_conditions(case, dense):
    """Ample memory: triangles, and the triangle-route rule (rows iff a quarter of the cells is occupied) gives the route the
    case stands for.  Tight memory (two slices): the bucket overflows and the same mesh comes out in pieces -- unless the
    vertex and index space of ONE slice of maximum cells, the least the constructor accepts, holds the whole bucket, so
    that no memory setting can make it overflow: the tube on W x 17 x 13 (13 % of 12 layers of cells, 7.6 vertices and 18.5
    indices a cell, 0.81 and 0.72 of one slice's space).  Its tight run is the ample one again and must say so."""
    _, st = mx.oracle_run(case, "ample")
    share = st["occupied"] / case.cells
    _, tight = mx.oracle_run(case, "tight")
    print("%s: %d x %d x %d, nw %d, occupied %.3f, %d triangles; tight: %d ship-outs, %d overflows"
          % ((case.name,) + case.size + (mx.lattice_words(case.size[0]), share, st["indices"] // 3, tight["shipouts"],
                                         tight["overflows"])))
    assert st["indices"] >= 3 * 100
    assert (st["occupied"] * 4 >= case.cells) == dense, (case.name, share)
    assert st["overflows"] == 0
    assert tight["indices"] == st["indices"] and tight["occupied"] == st["occupied"]
    slice_cells = (case.dims[0] - 1) * (case.dims[1] - 1)
    one_slice_holds_it = st["unwelded"] <= 13 * slice_cells and st["indices"] <= 36 * slice_cells
    assert not (dense and one_slice_holds_it)
    if one_slice_holds_it:
        assert tight["overflows"] == 0 and tight["shipouts"] == 1
    else:
        assert tight["overflows"] >= 1 and tight["shipouts"] > st["shipouts"]
    return st, tight


@pytest.mark.parametrize("width", sorted(mx.WIDTHS))
@pytest.mark.parametrize("field", ["noise", "tube"])
def test_width_case_conditions(field, width):
    check_conditions(mx.width_case(field, width), mx.DENSE[field])
    if width in mx.REGIME_WIDTHS:
        check_conditions(mx.width_case(field, width, sort_buffers=True), mx.DENSE[field])


@pytest.mark.parametrize("case", mx.EXTENT_CASES, ids=repr)
def test_extent_case_conditions(case):
    st, tight = check_conditions(case, mx.DENSE[case.field])
    if case.name == "deep_swathes":
        assert tight["overflows"] == 17                     # one for every swathe of 64 slices
    assert (case.max_swathe < case.size[2]) == ("swathes" in case.name)     # several swathes: the sort weld


def test_batch_lane_conditions():
    for case in mx.BATCH_B:
        if case.field == "positive":
            assert mx.oracle_run(case, "ample") == ([], dict.fromkeys(mx.oracle_run(case, "ample")[1], 0))
        else:
            check_conditions(case, mx.DENSE[case.field])
    assert [mx.lattice_words(c.size[0]) for c in mx.BATCH_B] == [64, 4, 33, 2, 65]
    assert len({c.dims for c in mx.BATCH_B}) == len(mx.BATCH_B)         # objects of different maximum sizes
