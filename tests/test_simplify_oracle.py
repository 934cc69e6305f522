"""The simplifier's CPU oracle (simplify_cases.py) pinned by answers that can be derived by hand, and the CPU-side checks of
the C-ABI of mlsgpu_hip_mesh_simplify / mlsgpu_hip_mesher_simplify."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import simplify_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_simplify", "mlsgpu_hip_mesher_simplify")


def test_grid_4x4_collapsed_2x2():
    p, tri = sc.grid_mesh(4, 4)
    v, t, st = sc.simplify(p, tri, (-0.5, -0.5, -0.5), 2.0)
    assert v.tolist() == [[0.5, 0.5, 0.0], [2.5, 0.5, 0.0], [0.5, 2.5, 0.0], [2.5, 2.5, 0.0]]
    # the centre quad (1, 1) (2, 1) (2, 2) (1, 2) of the input: its two triangles, oriented as tc.grid makes them
    assert tri[8].tolist() == [5, 9, 10] and tri[9].tolist() == [5, 10, 6]
    assert t.tolist() == [[0, 1, 3], [0, 3, 2]]
    assert st == dict(inVertices=16, inTriangles=18, outVertices=4, outTriangles=2, collapsedTriangles=16, duplicateTriangles=0)


def test_lossless_below_the_vertex_spacing():
    p, tri = sc.grid_mesh(7, 5, jitter=0.2, seed=3)
    p = np.concatenate([p, [[100.0, 100.0, 100.0]]]).astype(np.float32)       # a vertex nothing uses
    v, t, st = sc.simplify(p, tri, (-1.0, -1.0, -1.0), 0.25)
    assert st["outVertices"] == 35 and st["outTriangles"] == len(tri) and st["collapsedTriangles"] == st["duplicateTriangles"] == 0
    # every referenced vertex bit for bit: the output is a permutation of the 35
    got = sorted(map(tuple, v.view(np.uint32).tolist()))
    assert got == sorted(map(tuple, p[:35].view(np.uint32).tolist()))
    # and the triangles are the input's, re-indexed through that permutation
    where = dict((tuple(row), k) for k, row in enumerate(v.view(np.uint32).tolist()))
    perm = np.array([where[tuple(row)] for row in p[:35].view(np.uint32).tolist()])
    assert sc.canonical(t) == sc.canonical(perm[tri])
    # ascending (first, second, third)
    assert t.tolist() == sorted(t.tolist())


def test_everything_in_one_cell():
    p, tri = sc.grid_mesh(6, 6)
    v, t, st = sc.simplify(p, tri, (-1.0, -1.0, -1.0), 100.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)
    assert st == dict(inVertices=36, inTriangles=50, outVertices=0, outTriangles=0, collapsedTriangles=50, duplicateTriangles=0)


def test_thin_torus_has_duplicates():
    """A tube of radius 0.1 in cells of 2.5 whose boundary z = 0 cuts it lengthwise.  One clean winding has no duplicates,
    and provably so: triangles that map to the same three clusters lie on opposite sides of the tube and face opposite ways.
    Wound around the axis twice, the two layers face the same way."""
    p, tri = sc.torus_mesh(96, 6, 10.0, 0.1)
    assert sc.simplify(p, tri, (-12.5, -12.5, -12.5), 2.5)[2]["duplicateTriangles"] == 0
    p, tri = sc.torus_mesh(97, 6, 10.0, 0.1, windings=2)
    v, t, st = sc.simplify(p, tri, (-12.5, -12.5, -12.5), 2.5)
    assert st["duplicateTriangles"] > 0 and st["outTriangles"] > 0
    assert st["inTriangles"] == st["outTriangles"] + st["collapsedTriangles"] + st["duplicateTriangles"] == len(tri)
    assert len(set(map(tuple, t.tolist()))) == len(t) and t.max() == len(v) - 1


def test_empty_meshes_and_errors():
    p, tri = sc.grid_mesh(3, 3)
    for vv, tt in ((p[:0], tri[:0]), (p, tri[:0])):
        v, t, st = sc.simplify(vv, tt, (-1, -1, -1), 1.0)
        assert len(v) == 0 and len(t) == 0 and st["inVertices"] == len(vv) and st["outVertices"] == 0
    bad = p.copy()
    bad[4, 1] = np.nan
    for args in ((bad, tri, (-1, -1, -1), 1.0), (p, tri, (0.5, -1, -1), 1.0), (p, tri, (-1, -1, -1), 0.0),
                 (p, tri, (-1, -1, -1), -1.0), (p, tri, (-1, -1, -1), np.inf), (p, tri, (-1, np.inf, -1), 1.0),
                 (p, np.concatenate([tri, [[0, 1, 9]]]), (-1, -1, -1), 1.0)):
        with pytest.raises(sc.Invalid):
            sc.simplify(*args)
    far = p.copy()
    far[0, 0] = 2.0 ** 21 - 1                               # cell 2^21 from an origin of -1: one too many
    with pytest.raises(sc.Invalid):
        sc.simplify(far, tri, (-1, -1, -1), 1.0)
    far[0, 0] = 2.0 ** 21 - 2                               # the last cell
    assert sc.simplify(far, tri, (-1, -1, -1), 1.0)[2]["outTriangles"] == len(tri)


# ---------------------------------------------------------------- ABI

def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    asserted = re.findall(r"static_assert\(sizeof\(mlsgpu_simplify_stats\) == (\d+)", header())
    assert asserted == ["48"]
    assert C.sizeof(b.SimplifyStats) == 48
    assert tuple(f[0] for f in b.SimplifyStats._fields_) == sc.STAT_NAMES
    fields = re.search(r"typedef struct mlsgpu_simplify_stats\s*\{(.*?)\}\s*mlsgpu_simplify_stats;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert tuple(names) == sc.STAT_NAMES


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name


def test_argument_checks_need_no_gpu():
    """A NULL context, mesher or output is refused before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.SimplifyStats()
    origin = (C.c_float * 3)(0, 0, 0)
    assert L.mlsgpu_hip_mesh_simplify(None, None, 0, None, 0, origin, 1.0, None, None, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
    assert L.mlsgpu_hip_mesher_simplify(None, origin, 1.0, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
