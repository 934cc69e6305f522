"""CPU-side checks of the hole filling C-ABI: struct layout, symbols, the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import fill_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_fill_holes", "mlsgpu_hip_mesher_fill_holes")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    asserted = re.findall(r"static_assert\(sizeof\(mlsgpu_fill_stats\) == (\d+)", header())
    assert asserted == ["120"]
    assert re.search(r"typedef char mlsgpu_fill_stats_size_is_120\[sizeof\(mlsgpu_fill_stats\) == 120 \? 1 : -1\]", header())
    assert C.sizeof(b.FillStats) == 120
    fields = re.search(r"typedef struct mlsgpu_fill_stats\s*\{(.*?)\}\s*mlsgpu_fill_stats;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in fields.split(";") if decl.strip()]
    names = [n.strip() for _, rest in decls for n in rest.split(",")]
    assert names == [f[0] for f in b.FillStats._fields_] == list(fc.STAT_NAMES)
    kinds = [kind for kind, rest in decls for _ in rest.split(",")]
    ctype = dict(uint64_t=C.c_uint64, int64_t=C.c_int64)
    assert [ctype[k] for k in kinds] == [f[1] for f in b.FillStats._fields_]
    assert kinds == ["uint64_t"] * 14 + ["int64_t"]
    st = b.FillStats(filledLoops=7, scaleExponent=-3).as_dict()
    assert st["filledLoops"] == 7 and st["scaleExponent"] == -3 and all(isinstance(x, int) for x in st.values())


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors, and the limit of maxEdges."""
    from mlsgpu_amd import binding as b
    names = [f[0] for f in b.FillStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_fill_stats), %s);\n'
                   'printf("%%u\\n", MLSGPU_FILL_MAX_EDGES);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_fill_stats, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    first, second = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in first.split()] == [120] + [getattr(b.FillStats, n).offset for n in names]
    assert int(second) == b.FILL_MAX_EDGES == fc.MAX_EDGES_LIMIT == 2 ** 20


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    for name in ("mesh_fill_holes", "mesher_fill_holes"):
        assert callable(getattr(b, name)) and getattr(mlsgpu_amd, name) is getattr(b, name), name
    assert callable(b.Mesher.fill_holes) and mlsgpu_amd.FillStats is b.FillStats
    hpp = open(os.path.join(ROOT, "mlsgpu_amd", "host", "mlsgpu_hip.hpp")).read()
    for name in SYMBOLS:
        assert name in hpp, name


def test_argument_checks_need_no_gpu():
    """A NULL context / mesher / stats is refused before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.FillStats()
    assert L.mlsgpu_hip_mesh_fill_holes(None, None, 0, None, 0, 8, None, None, 0, None, 0, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
    assert L.mlsgpu_hip_mesher_fill_holes(None, 8, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
