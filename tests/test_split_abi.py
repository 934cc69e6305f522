"""CPU-side checks of the edge split's C-ABI: struct layout, symbols, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import split_cases as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_split_edges", "mlsgpu_hip_mesher_split_edges")
FLOATS = ("minQualityBefore", "minQualityAfter", "maxLengthSqBefore", "maxLengthSqAfter")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd.split_stats import SplitStats
    assert re.findall(r"static_assert\(sizeof\(mlsgpu_split_stats\) == (\d+)", header()) == ["424"]
    assert re.search(r"typedef char mlsgpu_split_stats_size_is_424\[sizeof\(mlsgpu_split_stats\) == 424 \? 1 : -1\]", header())
    assert C.sizeof(SplitStats) == 424
    assert [f[0] for f in SplitStats._fields_] == list(sp.STAT_NAMES)
    st = SplitStats(splits=7, boundarySplits=2, converged=1, limited=1, minQualityAfter=0.25, maxLengthSqBefore=9.0)
    st.qualityBefore[15] = 5
    st.qualityAfter[0] = 3
    d = st.as_dict()
    assert list(d) == list(sp.STAT_NAMES)
    assert d == dict(sp.empty_stats(), splits=7, boundarySplits=2, converged=1, limited=1, minQualityAfter=0.25, maxLengthSqBefore=9.0,
                     qualityBefore=[0] * 15 + [5], qualityAfter=[3] + [0] * 15)
    assert all(type(d[name]) is (float if name in FLOATS else list if name.startswith("quality") else int) for name in d)


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors."""
    from mlsgpu_amd.split_stats import SplitStats
    names = [f[0] for f in SplitStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_split_stats), %s);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_split_stats, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in out] == [424] + [getattr(SplitStats, n).offset for n in names]


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b, split_stats
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    hpp = open(os.path.join(ROOT, "mlsgpu_amd", "host", "mlsgpu_hip.hpp")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
        assert name in hpp, name
    assert L.mlsgpu_hip_mesh_split_edges.argtypes[5:8] == [C.c_uint32, C.c_double, C.c_uint64] and len(L.mlsgpu_hip_mesh_split_edges.argtypes) == 15
    assert L.mlsgpu_hip_mesher_split_edges.argtypes[1:4] == [C.c_uint32, C.c_double, C.c_uint32]
    assert callable(b.mesh_split_edges) and mlsgpu_amd.mesh_split_edges is b.mesh_split_edges
    assert callable(b.Mesher.split_edges)
    assert mlsgpu_amd.SplitStats is split_stats.SplitStats and issubclass(split_stats.SplitStats, b.Stats)
    assert not hasattr(b, "SplitStats")         # test_stats_dict.py lists every statistics structure of binding's own namespace
    assert hpp.count("splitEdges") >= 2
    makefile = open(os.path.join(ROOT, "mlsgpu_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\bsplit\.o\b", makefile, re.M)


def test_argument_checks_need_no_gpu():
    """A NULL context / mesher / statistics comes back before any device work."""
    from mlsgpu_amd import binding as b
    from mlsgpu_amd.split_stats import SplitStats
    L = b.lib()
    st = SplitStats()
    for call in (lambda: L.mlsgpu_hip_mesh_split_edges(None, None, 0, None, 0, 4, 0.1, 0, None, None, 0, None, 0, None, C.byref(st)),
                 lambda: L.mlsgpu_hip_mesh_split_edges(None, None, 0, None, 0, 4, 0.1, 0, None, None, 0, None, 0, None, None),
                 lambda: L.mlsgpu_hip_mesher_split_edges(None, 4, 0.1, 0, C.byref(st)),
                 lambda: L.mlsgpu_hip_mesher_split_edges(None, 4, 0.1, 0, None)):
        assert call() == 1
        assert b"requirement failed" in L.mlsgpu_hip_last_error()
