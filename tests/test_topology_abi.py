"""CPU-side checks of the topology report's C-ABI: struct layout, symbols, and the host-only reason text."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_topology", "mlsgpu_hip_mesher_chunk_topology", "mlsgpu_hip_topology_reason")


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    asserted = re.findall(r"static_assert\(sizeof\(mlsgpu_topology\) == (\d+)", header())
    assert len(asserted) == 1
    assert C.sizeof(b.Topology) == int(asserted[0])
    fields = re.search(r"typedef struct mlsgpu_topology\s*\{(.*?)\}\s*mlsgpu_topology;", header(), re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = [n.strip().split("[")[0] for decl in fields.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f[0] for f in b.Topology._fields_]
    for k, name in enumerate(("OUT_OF_RANGE", "DEGENERATE", "ISOLATED", "DUPLICATED", "MIXED", "TUNNEL", "NONE")):
        assert re.search(r"#define MLSGPU_TOPO_%s %d\b" % (name, k), header()), name
        assert getattr(b, "TOPO_" + name) == k


def test_symbols_are_declared_exported_and_bound():
    import mlsgpu_amd
    raw = C.CDLL(mlsgpu_amd.library_path())
    L = mlsgpu_amd.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header()), name
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name


def hand_filled(kind, index):
    from mlsgpu_amd import binding as b
    t = b.Topology()
    t.firstKind, t.firstIndex, t.manifold = kind, index, int(kind == b.TOPO_NONE)
    return t


def test_reason_text_without_a_gpu():
    """One sentence per class, in the wording of test/manifold.h:121-216 (the report names a vertex for a repeated edge and
    does not carry a bad triangle's offending index); "" for a manifold mesh."""
    from mlsgpu_amd import binding as b
    assert b.reason(hand_filled(b.TOPO_NONE, 2 ** 64 - 1)) == ""
    want = {b.TOPO_OUT_OF_RANGE: "Triangle 7 contains an out-of-range index",
            b.TOPO_DEGENERATE: "Triangle 7 contains a vertex twice",
            b.TOPO_ISOLATED: "Vertex 7 is isolated",
            b.TOPO_DUPLICATED: "Vertex 7 is on an edge that occurs twice with same winding",
            b.TOPO_MIXED: "Vertex 7 is both in the interior and on the boundary",
            b.TOPO_TUNNEL: "Vertex 7 tunnels between interior regions"}
    for kind, text in want.items():
        assert b.reason(hand_filled(kind, 7)) == text
    # the reference's own words where the report can say them (tests/refdata.py restates its messages)
    from refdata import is_manifold
    assert is_manifold(4, []) == b.reason(hand_filled(b.TOPO_ISOLATED, 0))
    assert b.reason(hand_filled(b.TOPO_ISOLATED, 4294967295 * 3)) == "Vertex 12884901885 is isolated"
    # the C contract: the whole length is returned, a short buffer gets a terminated prefix, NULL is allowed
    L = b.lib()
    t = hand_filled(b.TOPO_TUNNEL, 7)
    full = want[b.TOPO_TUNNEL]
    assert L.mlsgpu_hip_topology_reason(C.byref(t), None, 0) == len(full)
    buf = C.create_string_buffer(b"\xff" * 16, 16)
    assert L.mlsgpu_hip_topology_reason(C.byref(t), buf, 9) == len(full)
    assert buf.raw[:9] == full[:8].encode() + b"\0" and buf.raw[9:] == b"\xff" * 7


def test_argument_checks_need_no_gpu():
    """NULL context / output and sizes beyond 32 bits are refused before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    t = b.Topology()
    assert L.mlsgpu_hip_mesh_topology(None, None, 0, 0, C.byref(t)) == 1
    assert L.mlsgpu_hip_mesher_chunk_topology(None, 0, C.byref(t)) == 1
    assert b"requirement failed" in L.mlsgpu_hip_last_error()
