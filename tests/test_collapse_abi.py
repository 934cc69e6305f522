"""CPU-side checks of the edge collapse's C-ABI: struct layout, symbols, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import collapse_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_collapse_edges", "mlsgpu_hip_mesher_collapse_edges")
FLOATS = ("minQualityBefore", "minQualityAfter", "minLengthSqBefore", "minLengthSqAfter")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    assert re.findall(r"static_assert\(sizeof\(mlsgpu_collapse_stats\) == (\d+)", header()) == ["416"]
    assert re.search(r"typedef char mlsgpu_collapse_stats_size_is_416\[sizeof\(mlsgpu_collapse_stats\) == 416 \? 1 : -1\]", header())
    assert re.findall(r"#define MLSGPU_COLLAPSE_MAX_VALENCE (\d+)u", header()) == [str(cc.MAX_VALENCE)]
    assert C.sizeof(b.CollapseStats) == 416
    assert [f[0] for f in b.CollapseStats._fields_] == list(cc.STAT_NAMES)
    st = b.CollapseStats(collapses=7, converged=1, minQualityAfter=0.25, minLengthSqBefore=float("inf"), minLengthSqAfter=float("inf"))
    st.qualityBefore[15] = 5
    st.qualityAfter[0] = 3
    d = st.as_dict()
    assert list(d) == list(cc.STAT_NAMES)
    assert d == dict(cc.empty_stats(), collapses=7, converged=1, minQualityAfter=0.25, qualityBefore=[0] * 15 + [5],
                     qualityAfter=[3] + [0] * 15)
    assert all(type(d[name]) is (float if name in FLOATS else list if name.startswith("quality") else int) for name in d)


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors."""
    from mlsgpu_amd import binding as b
    names = [f[0] for f in b.CollapseStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_collapse_stats), %s);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_collapse_stats, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in out] == [416] + [getattr(b.CollapseStats, n).offset for n in names]


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    hpp = open(os.path.join(ROOT, "mlsgpu_amd", "host", "mlsgpu_hip.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
        assert name in hpp, name
    assert L.mlsgpu_hip_mesh_collapse_edges.argtypes[6:8] == [C.c_double, C.c_double]
    assert L.mlsgpu_hip_mesher_collapse_edges.argtypes[2:4] == [C.c_double, C.c_double]
    assert callable(b.mesh_collapse_edges) and mlsgpu_amd.mesh_collapse_edges is b.mesh_collapse_edges
    assert callable(b.Mesher.collapse_edges)
    assert mlsgpu_amd.CollapseStats is b.CollapseStats
    assert "collapseEdges" in hpp
    makefile = open(os.path.join(ROOT, "mlsgpu_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\bcollapse\.o\b", makefile, re.M)


def test_argument_checks_need_no_gpu():
    """A NULL context / mesher / statistics comes back before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.CollapseStats()
    for call in (lambda: L.mlsgpu_hip_mesh_collapse_edges(None, None, 0, None, 0, 4, 0.1, 0.5, None, 0, None, 0, None, C.byref(st)),
                 lambda: L.mlsgpu_hip_mesh_collapse_edges(None, None, 0, None, 0, 4, 0.1, 0.5, None, 0, None, 0, None, None),
                 lambda: L.mlsgpu_hip_mesher_collapse_edges(None, 4, 0.1, 0.5, C.byref(st)),
                 lambda: L.mlsgpu_hip_mesher_collapse_edges(None, 4, 0.1, 0.5, None)):
        assert call() == 1
        assert b"requirement failed" in L.mlsgpu_hip_last_error()
