"""CPU-side checks of the deviation report's C-ABI: struct layout, symbols, the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import deviation_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_deviation", "mlsgpu_hip_mesher_keep_reference", "mlsgpu_hip_mesher_drop_reference",
           "mlsgpu_hip_mesher_deviation")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    asserted = re.findall(r"static_assert\(sizeof\(mlsgpu_deviation\) == (\d+)", header())
    assert asserted == ["232"]
    assert re.search(r"typedef char mlsgpu_deviation_size_is_232\[sizeof\(mlsgpu_deviation\) == 232 \? 1 : -1\]", header())
    assert C.sizeof(b.Deviation) == 232
    fields = re.search(r"typedef struct mlsgpu_deviation\s*\{(.*?)\}\s*mlsgpu_deviation;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in fields.split(";") if decl.strip()]
    declared = [(kind, n.strip()) for kind, rest in decls for n in rest.split(",")]
    names = [re.sub(r"\[\d+\]", "", n) for _, n in declared]
    assert names == [f[0] for f in b.Deviation._fields_] == list(dc.STAT_NAMES)
    ctype = dict(uint64_t=C.c_uint64, int64_t=C.c_int64, double=C.c_double)
    kinds = [ctype[kind] * int(n[n.index("[") + 1:-1]) if "[" in n else ctype[kind] for kind, n in declared]
    assert [(k._type_, k._length_) if hasattr(k, "_length_") else k for k in kinds] == \
        [(f[1]._type_, f[1]._length_) if hasattr(f[1], "_length_") else f[1] for f in b.Deviation._fields_]
    assert [kind for kind, _ in declared] == ["uint64_t"] * 10 + ["int64_t"] * 2 + ["double"] * 2
    st = b.Deviation(within=7, scaleExponent=-3, sumQ=5 << 33, maxDistance2=0.25, limit2=1.0)
    st.histogram[15] = 9
    d = st.as_dict()
    assert d["within"] == 7 and d["scaleExponent"] == -3 and d["histogram"] == [0] * 15 + [9] and d["maxDistance2"] == 0.25
    assert all(isinstance(d[k], int) for k in dc.STAT_NAMES[:9] + ("sumQ", "scaleExponent")) and isinstance(d["limit2"], float)
    assert d["meanSquare"] == dc.mean_square(d) == 5.0 / 7


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors."""
    from mlsgpu_amd import binding as b
    names = [f[0] for f in b.Deviation._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_deviation), %s);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_deviation, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in out] == [232] + [getattr(b.Deviation, n).offset for n in names]


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    for name in ("mesh_deviation", "mesher_deviation"):
        assert callable(getattr(b, name)) and getattr(mlsgpu_amd, name) is getattr(b, name), name
    for name in ("keep_reference", "drop_reference", "deviation"):
        assert callable(getattr(b.Mesher, name)), name
    assert mlsgpu_amd.Deviation is b.Deviation
    hpp = open(os.path.join(ROOT, "mlsgpu_amd", "host", "mlsgpu_hip.hpp")).read()
    for name in SYMBOLS:
        assert name in hpp, name


def test_argument_checks_need_no_gpu():
    """A NULL context / mesher / report is refused before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.Deviation()
    assert L.mlsgpu_hip_mesh_deviation(None, None, 0, None, 0, None, 0, 1.0, None, None, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
    for call in (lambda: L.mlsgpu_hip_mesher_keep_reference(None), lambda: L.mlsgpu_hip_mesher_drop_reference(None),
                 lambda: L.mlsgpu_hip_mesher_deviation(None, 1.0, C.byref(st), C.byref(st))):
        assert call() == 1
        assert b"requirement failed" in L.mlsgpu_hip_last_error()
