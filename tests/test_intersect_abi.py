"""CPU-side checks of the self-intersection report's C-ABI: struct layout, symbols, the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import intersect_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_self_intersections", "mlsgpu_hip_mesher_self_intersections")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    asserted = re.findall(r"static_assert\(sizeof\(mlsgpu_self_intersections\) == (\d+)", header())
    assert asserted == ["104"]
    assert re.search(r"typedef char mlsgpu_self_intersections_size_is_104\[sizeof\(mlsgpu_self_intersections\) == 104 \? 1 : -1\]",
                     header())
    assert C.sizeof(b.SelfIntersections) == 104
    fields = re.search(r"typedef struct mlsgpu_self_intersections\s*\{(.*?)\}\s*mlsgpu_self_intersections;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in fields.split(";") if decl.strip()]
    declared = [(kind, n.strip()) for kind, rest in decls for n in rest.split(",")]
    assert [n for _, n in declared] == [f[0] for f in b.SelfIntersections._fields_] == list(ic.STAT_NAMES)
    assert [kind for kind, _ in declared] == ["uint64_t"] * 13
    assert all(f[1] is C.c_uint64 for f in b.SelfIntersections._fields_)
    st = b.SelfIntersections(crossingPairs=7, lowestA=ic.NONE, maxPartnersTriangle=3, crossingChunks=2)
    d = st.as_dict()
    assert list(d) == list(ic.STAT_NAMES) and all(isinstance(v, int) for v in d.values())
    assert (d["crossingPairs"], d["lowestA"], d["maxPartnersTriangle"], d["crossingChunks"]) == (7, ic.NONE, 3, 2)


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors."""
    from mlsgpu_amd import binding as b
    names = [f[0] for f in b.SelfIntersections._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_self_intersections), %s);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_self_intersections, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in out] == [104] + [getattr(b.SelfIntersections, n).offset for n in names]


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    for name in ("mesh_self_intersections", "mesher_self_intersections"):
        assert callable(getattr(b, name)) and getattr(mlsgpu_amd, name) is getattr(b, name), name
    assert callable(b.Mesher.self_intersections)
    assert mlsgpu_amd.SelfIntersections is b.SelfIntersections
    hpp = open(os.path.join(ROOT, "mlsgpu_amd", "host", "mlsgpu_hip.hpp")).read()
    for name in SYMBOLS:
        assert name in hpp, name
    makefile = open(os.path.join(ROOT, "mlsgpu_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\bintersect\.o\b", makefile, re.M)


def test_argument_checks_need_no_gpu():
    """A NULL context / mesher / report, and lengths beyond 32 bits, are refused before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.SelfIntersections()
    assert L.mlsgpu_hip_mesh_self_intersections(None, None, 0, None, 0, None, None, 0, C.byref(st)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
    for call in (lambda: L.mlsgpu_hip_mesher_self_intersections(None, C.byref(st)),
                 lambda: L.mlsgpu_hip_mesher_self_intersections(None, None)):
        assert call() == 1
        assert b"requirement failed" in L.mlsgpu_hip_last_error()
