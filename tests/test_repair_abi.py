"""CPU-side checks of the mesh repair C-ABI: struct layout, symbols, the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import repair_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_repair", "mlsgpu_hip_mesher_repair")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    asserted = re.findall(r"static_assert\(sizeof\(mlsgpu_repair_stats\) == (\d+)", header())
    assert asserted == ["88"]
    assert re.search(r"typedef char mlsgpu_repair_stats_size_is_88\[sizeof\(mlsgpu_repair_stats\) == 88 \? 1 : -1\]", header())
    assert C.sizeof(b.RepairStats) == 88
    fields = re.search(r"typedef struct mlsgpu_repair_stats\s*\{(.*?)\}\s*mlsgpu_repair_stats;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    decls = [decl.strip().split(None, 1) for decl in fields.split(";") if decl.strip()]
    names = [n.strip() for _, rest in decls for n in rest.split(",")]
    assert names == [f[0] for f in b.RepairStats._fields_] == list(rc.STAT_NAMES)
    kinds = [kind for kind, rest in decls for _ in rest.split(",")]
    assert kinds == ["uint64_t"] * 11 and all(f[1] is C.c_uint64 for f in b.RepairStats._fields_)
    st = b.RepairStats(droppedTriangles=7, addedVertices=3).as_dict()
    assert st["droppedTriangles"] == 7 and st["addedVertices"] == 3 and all(isinstance(x, int) for x in st.values())
    assert list(st) == list(rc.STAT_NAMES)


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors, and the flag."""
    from mlsgpu_amd import binding as b
    names = [f[0] for f in b.RepairStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_repair_stats), %s);\n'
                   'printf("%%u\\n", MLSGPU_REPAIR_SPLIT_PINCHES);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_repair_stats, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    first, second = subprocess.check_output([str(exe)]).decode().splitlines()
    assert [int(x) for x in first.split()] == [88] + [getattr(b.RepairStats, n).offset for n in names]
    assert [getattr(b.RepairStats, n).offset for n in names] == list(range(0, 88, 8))
    assert int(second) == b.REPAIR_SPLIT_PINCHES == rc.SPLIT_PINCHES == 1


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    from mlsgpu_amd import binding as b
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name
    for name in ("mesh_repair", "mesher_repair"):
        assert callable(getattr(b, name)) and getattr(mlsgpu_amd, name) is getattr(b, name), name
    assert callable(b.Mesher.repair) and mlsgpu_amd.RepairStats is b.RepairStats
    assert mlsgpu_amd.REPAIR_SPLIT_PINCHES == 1
    hpp = open(os.path.join(ROOT, "mlsgpu_amd", "host", "mlsgpu_hip.hpp")).read()
    for name in SYMBOLS:
        assert name in hpp, name
    assert "repair.o" in open(os.path.join(ROOT, "mlsgpu_amd", "csrc", "Makefile")).read()


def test_argument_checks_need_no_gpu():
    """A NULL context / mesher / stats and an unknown flag bit are refused before any device work.  The flag is checked before
    the handle is looked at, so a block of zero bytes stands in for a context and a mesher here."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.RepairStats()
    stand_in = C.create_string_buffer(4096)
    handle = C.cast(stand_in, C.c_void_p)

    def refused(rc_):
        assert rc_ == 1
        assert b"requirement failed" in L.mlsgpu_hip_last_error()

    refused(L.mlsgpu_hip_mesh_repair(None, None, 0, None, 0, 0, None, 0, None, 0, None, C.byref(st)))
    refused(L.mlsgpu_hip_mesh_repair(handle, None, 0, None, 0, 0, None, 0, None, 0, None, None))
    for flags in (2, 3, 1 << 31):
        refused(L.mlsgpu_hip_mesh_repair(handle, None, 0, None, 0, flags, None, 0, None, 0, None, C.byref(st)))
        refused(L.mlsgpu_hip_mesher_repair(handle, flags, C.byref(st)))
    refused(L.mlsgpu_hip_mesher_repair(None, 0, C.byref(st)))
    refused(L.mlsgpu_hip_mesher_repair(handle, 0, None))
    # sizes beyond 32-bit indices: MLSGPU_ERR_LENGTH before anything is allocated or the context is used
    for nv, nt in ((1 << 32, 0), (0, ((1 << 32) + 2) // 3)):
        assert L.mlsgpu_hip_mesh_repair(handle, handle, nv, handle, nt, 0, None, 0, None, 0, None, C.byref(st)) == 2
    assert bytes(stand_in) == bytes(4096)
