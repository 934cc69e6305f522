"""CPU-side checks of the vertex-normal C-ABI: struct layout, symbols, argument checks, and the host PLY writer with normals
byte for byte (beside the plain writer's file, which must not change)."""
import ctypes as C
import os
import re

import numpy as np

import normals_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_normals", "mlsgpu_hip_mesher_chunk_normals", "mlsgpu_hip_write_ply_normals",
           "mlsgpu_hip_mesher_write_ply_normals", "mlsgpu_hip_write_ply")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    asserted = re.findall(r"static_assert\(sizeof\(mlsgpu_normals_stats\) == (\d+)", header())
    assert asserted == ["48"]
    assert re.search(r"typedef char mlsgpu_normals_stats_size_is_48\[sizeof\(mlsgpu_normals_stats\) == 48 \? 1 : -1\]", header())
    assert C.sizeof(b.NormalsStats) == 48
    fields = re.search(r"typedef struct mlsgpu_normals_stats\s*\{(.*?)\}\s*mlsgpu_normals_stats;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in b.NormalsStats._fields_] == list(nc.STAT_NAMES)
    assert b.NormalsStats._fields_[-1][1] is C.c_int64


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    for name in ("mesh_normals", "mesher_chunk_normals", "write_ply_normals", "mesher_write_ply_normals"):
        assert callable(getattr(b, name)), name


def test_argument_checks_need_no_gpu():
    """NULL context / mesher and sizes beyond 32 bits are refused before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.NormalsStats()
    assert L.mlsgpu_hip_mesh_normals(None, None, 0, None, 0, None, C.byref(st)) == 1
    assert L.mlsgpu_hip_mesher_chunk_normals(None, 0, None, C.byref(st)) == 1
    assert L.mlsgpu_hip_mesher_write_ply_normals(None, 0, b"/nonexistent/x.ply", None, 0, 0) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()


def assembled(vertices, triangles, comments, normals=None):
    """FastPly::Writer's file, put together here: the header text padded to a multiple of four, the vertex rows, the faces."""
    head = "ply\nformat binary_little_endian 1.0\n" + "".join("comment %s\n" % c for c in comments)
    head += "element vertex %d\nproperty float32 x\nproperty float32 y\nproperty float32 z\n" % len(vertices)
    if normals is not None:
        head += "property float32 nx\nproperty float32 ny\nproperty float32 nz\n"
    head += "element face %d\nproperty list uint8 uint32 vertex_indices\ncomment padding:" % len(triangles)
    head += "X" * (-(len(head) + len("\nend_header\n")) % 4) + "\nend_header\n"
    assert len(head) % 4 == 0
    rows = vertices if normals is None else np.concatenate([vertices, normals], axis=1)
    faces = np.zeros(len(triangles), np.dtype([("n", np.uint8), ("i", "<u4", 3)]))
    faces["n"], faces["i"] = 3, triangles
    return head.encode("ascii") + np.ascontiguousarray(rows, "<f4").tobytes() + faces.tobytes()


def test_host_writers_byte_for_byte(tmp_path):
    from mlsgpu_amd import binding as b
    p, tri = nc.grid_mesh(5, 7, jitter=0.3, seed=4)
    n, _ = nc.normals(p, tri)
    tri = tri.astype(np.uint32)
    for comments in [(), ("a",), ("ab",), ("abc",), ("mlsgpu-hip", "two words")]:      # comment bytes of every remainder mod 4
        b.write_ply_normals(tmp_path / "normals.ply", p, n, tri, comments=comments)
        assert (tmp_path / "normals.ply").read_bytes() == assembled(p, tri, comments, n), comments
        b.write_ply(tmp_path / "plain.ply", p, tri, comments=comments)
        assert (tmp_path / "plain.ply").read_bytes() == assembled(p, tri, comments), comments
    b.write_ply_normals(tmp_path / "empty.ply", p[:0], n[:0], tri[:0])
    assert (tmp_path / "empty.ply").read_bytes() == assembled(p[:0], tri[:0], (), n[:0])
