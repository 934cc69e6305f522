"""CPU-side checks of the quadric-placement C-ABI: the struct's layout in the header, in C and in ctypes, the symbols, and the
argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import simplify_quadric_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_simplify_quadric", "mlsgpu_hip_mesher_simplify_quadric")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_is_the_headers():
    from mlsgpu_amd import binding as b
    assert re.findall(r"static_assert\(sizeof\(mlsgpu_simplify_quadric_stats\) == (\d+)", header()) == ["80"]
    assert re.search(r"typedef char mlsgpu_simplify_quadric_stats_size_is_80\[sizeof\(mlsgpu_simplify_quadric_stats\) == 80 \? 1 : -1\]",
                     header())
    assert C.sizeof(b.SimplifyQuadricStats) == 80
    fields = re.search(r"typedef struct mlsgpu_simplify_quadric_stats\s*\{(.*?)\}\s*mlsgpu_simplify_quadric_stats;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in fields.split(";") if decl.strip()]
    names = [n.strip() for _, rest in decls for n in rest.split(",")]
    assert names == [f[0] for f in b.SimplifyQuadricStats._fields_] == list(qc.STAT_NAMES)
    assert names[:6] == [f[0] for f in b.SimplifyStats._fields_]
    kinds = [kind for kind, rest in decls for _ in rest.split(",")]
    assert kinds == ["uint64_t"] * 9 + ["int64_t"]
    assert [f[1] for f in b.SimplifyQuadricStats._fields_] == [C.c_uint64] * 9 + [C.c_int64]
    st = b.SimplifyQuadricStats(solvedVertices=7, scaleExponent=-3).as_dict()
    assert list(st) == list(qc.STAT_NAMES) and st["solvedVertices"] == 7 and st["scaleExponent"] == -3


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors."""
    from mlsgpu_amd import binding as b
    names = [f[0] for f in b.SimplifyQuadricStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_simplify_quadric_stats), %s);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_simplify_quadric_stats, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [80] + [getattr(b.SimplifyQuadricStats, n).offset for n in names]
    assert got[1:] == list(range(0, 80, 8))


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    assert callable(b.mesh_simplify_quadric) and mlsgpu_amd.mesh_simplify_quadric is b.mesh_simplify_quadric
    assert callable(b.Mesher.simplify_quadric) and mlsgpu_amd.SimplifyQuadricStats is b.SimplifyQuadricStats


def test_null_arguments_need_no_gpu():
    """A NULL context, mesher, origin or statistics block is refused before any device work.  (A bad cellSize and the 32-bit
    length rule are checked behind the context: test_gpu_simplify_quadric.py.)"""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st, origin = b.SimplifyQuadricStats(outVertices=5), (C.c_float * 3)(0.0, 0.0, 0.0)
    assert L.mlsgpu_hip_mesh_simplify_quadric(None, None, 0, None, 0, origin, 1.0, None, None, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
    assert L.mlsgpu_hip_mesher_simplify_quadric(None, origin, 1.0, C.byref(st)) == 1
    assert L.mlsgpu_hip_mesher_simplify_quadric(None, None, 1.0, None) == 1
    assert st.outVertices == 5              # a refused call leaves the block alone
