"""CPU-side checks of the smoothing C-ABI: struct layout, symbols, the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import smooth_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_smooth", "mlsgpu_hip_mesher_smooth")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    asserted = re.findall(r"static_assert\(sizeof\(mlsgpu_smooth_stats\) == (\d+)", header())
    assert asserted == ["96"]
    assert re.search(r"typedef char mlsgpu_smooth_stats_size_is_96\[sizeof\(mlsgpu_smooth_stats\) == 96 \? 1 : -1\]", header())
    assert C.sizeof(b.SmoothStats) == 96
    fields = re.search(r"typedef struct mlsgpu_smooth_stats\s*\{(.*?)\}\s*mlsgpu_smooth_stats;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in fields.split(";") if decl.strip()]
    names = [n.strip() for _, rest in decls for n in rest.split(",")]
    assert names == [f[0] for f in b.SmoothStats._fields_] == list(sc.STAT_NAMES)
    kinds = [kind for kind, rest in decls for _ in rest.split(",")]
    ctype = dict(uint64_t=C.c_uint64, int64_t=C.c_int64, double=C.c_double)
    assert [ctype[k] for k in kinds] == [f[1] for f in b.SmoothStats._fields_]
    assert kinds == ["uint64_t"] * 9 + ["int64_t"] + ["double"] * 2
    st = b.SmoothStats(maxMove=0.25, scaleExponent=-3).as_dict()
    assert st["maxMove"] == 0.25 and st["scaleExponent"] == -3 and isinstance(st["passes"], int) and isinstance(st["maxCoordinate"], float)


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors."""
    from mlsgpu_amd import binding as b
    names = [f[0] for f in b.SmoothStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_smooth_stats), %s);\n'
                   'printf("%%d %%d\\n", MLSGPU_SMOOTH_BOUNDARY_FIXED, MLSGPU_SMOOTH_BOUNDARY_CURVE);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_smooth_stats, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    first, second = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in first.split()] == [96] + [getattr(b.SmoothStats, n).offset for n in names]
    assert [int(x) for x in second.split()] == [b.SMOOTH_BOUNDARY_FIXED, b.SMOOTH_BOUNDARY_CURVE] == [sc.FIXED, sc.CURVE]


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    for name in ("mesh_smooth", "mesher_smooth"):
        assert callable(getattr(b, name)), name
    assert callable(b.Mesher.smooth) and mlsgpu_amd.mesh_smooth is b.mesh_smooth and mlsgpu_amd.SmoothStats is b.SmoothStats
    hpp = open(os.path.join(ROOT, "mlsgpu_amd", "host", "mlsgpu_hip.hpp")).read()
    for name in SYMBOLS:
        assert name in hpp, name


def test_argument_checks_need_no_gpu():
    """A NULL context / mesher / stats is refused before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.SmoothStats()
    assert L.mlsgpu_hip_mesh_smooth(None, None, 0, None, 0, 1, 0.5, -0.53, 0, None, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
    assert L.mlsgpu_hip_mesher_smooth(None, 1, 0.5, -0.53, 0, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
