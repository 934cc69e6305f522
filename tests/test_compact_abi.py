"""CPU-side checks of the compact read-back's C-ABI: struct layout, symbols, the argument checks that need no device, and the
host decoder -- against the oracle on well-formed blobs, and on every malformed one with guard bands around its outputs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compact_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mlsgpu_hip_mesh_compact", "mlsgpu_hip_mesher_chunk_compact", "mlsgpu_hip_compact_info", "mlsgpu_hip_compact_decode")
FORMAT = 7


def header():
    return open(os.path.join(ROOT, "include", "mlsgpu_hip.h")).read()


def test_struct_size_is_the_headers():
    from mlsgpu_amd import binding as b
    assert re.findall(r"static_assert\(sizeof\(mlsgpu_compact_stats\) == (\d+)", header()) == ["352"]
    assert re.search(r"typedef char mlsgpu_compact_stats_size_is_352\[sizeof\(mlsgpu_compact_stats\) == 352 \? 1 : -1\]", header())
    assert C.sizeof(b.CompactStats) == 352 == cc.STATS_BYTES
    assert [f[0] for f in b.CompactStats._fields_] == list(cc.STAT_NAMES)
    st = b.CompactStats(blobBytes=7, exceptions=3)
    st.widthHistogram[32] = 5
    st.step[2] = 0.5
    d = st.as_dict()
    assert list(d) == list(cc.STAT_NAMES)
    assert (d["blobBytes"], d["exceptions"], d["widthHistogram"][32], d["step"]) == (7, 3, 5, [0.0, 0.0, 0.5])
    for name, value in (("MAGIC", "0x43534C4Du"), ("VERSION", "1u"), ("GROUP", "64u"), ("HEADER_WORDS", "16u")):
        assert re.search(r"#define MLSGPU_COMPACT_%s %s\b" % (name, value), header()), name


def test_layout_is_the_c_compilers(tmp_path):
    """The header as plain C: the size and every offset of the struct the binding mirrors."""
    from mlsgpu_amd import binding as b
    names = [f[0] for f in b.CompactStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlsgpu_hip.h"\nint main(void) {\n'
                   'printf("%%zu %s\\n", sizeof(mlsgpu_compact_stats), %s);\nreturn 0; }\n'
                   % (" ".join(["%zu"] * len(names)), ", ".join("offsetof(mlsgpu_compact_stats, %s)" % n for n in names)))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(x) for x in out] == [352] + [getattr(b.CompactStats, n).offset for n in names]


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
    for name in ("mesh_compact", "compact_info", "compact_decode"):
        assert callable(getattr(b, name)) and getattr(mlsgpu_amd, name) is getattr(b, name), name
    assert callable(b.Mesher.chunk_compact)
    assert mlsgpu_amd.CompactStats is b.CompactStats
    makefile = open(os.path.join(ROOT, "mlsgpu_amd", "csrc", "Makefile")).read()
    assert re.search(r"^OBJS = .*\bcompact\.o\b", makefile, re.M)


def test_argument_checks_need_no_gpu():
    """A NULL context / mesher / statistics and a refused vertexBits come back before any device work."""
    from mlsgpu_amd import binding as b
    L = b.lib()
    st = b.CompactStats()
    calls = [lambda: L.mlsgpu_hip_mesh_compact(None, None, 0, None, 0, 32, None, 0, C.byref(st)),
             lambda: L.mlsgpu_hip_mesher_chunk_compact(None, 0, 32, None, 0, C.byref(st)),
             lambda: L.mlsgpu_hip_compact_info(None, 64, C.byref(st)),
             lambda: L.mlsgpu_hip_compact_decode(None, 64, None, None, 1)]
    blob = cc.encode(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), 32)[0]
    calls.append(lambda: L.mlsgpu_hip_compact_info(blob.ctypes.data, blob.nbytes, None))
    calls.append(lambda: L.mlsgpu_hip_compact_info(blob.ctypes.data + 1, blob.nbytes, C.byref(st)))     # misaligned
    for call in calls:
        assert call() == 1
        assert b"requirement failed" in L.mlsgpu_hip_last_error()


# ---------------------------------------------------------------- the decoder on well-formed blobs

@pytest.mark.parametrize("b", (8, 16, 21, 24, 32))
def test_decoder_equals_the_oracle(b):
    from mlsgpu_amd import binding as bd
    cases = [(cc.ring_vertices(V, V, offset=(1.0e6, -3.0, 0.0), scale=2.0), cc.local_triangles(T, max(V, 1), seed=T))
             for V, T in ((0, 0), (1, 1), (64, 63), (65, 64), (63, 65), (1000, 257), (5, 1000))]
    cases += [(np.zeros((0, 3), np.float32), t) for _, t, _, _, _ in cc.hand_cases()]
    for v, t in cases:
        blob, want = cc.encode(v, t, b)
        cc.same_stats(bd.compact_info(blob), want)
        cc.same_stats(bd.compact_info(blob.tobytes()), want)
        oracle_v, oracle_t = cc.decode(blob)
        for threads in (1, 3, 8):
            got_v, got_t = bd.compact_decode(blob, threads)
            assert got_t.tobytes() == t.tobytes() == oracle_t.tobytes()
            assert got_v.tobytes() == oracle_v.tobytes()                        # the decoder's arithmetic is the contract's
            cc.check_vertices(got_v, v, b)


def test_decoder_default_threads_and_many():
    from mlsgpu_amd import binding as bd
    v, t = cc.ring_vertices(3000, 1), cc.local_triangles(5000, 3000)
    blob, _ = cc.encode(v, t, 16)
    want = cc.decode(blob)
    for threads in (0, 64, 1000):
        got = bd.compact_decode(blob, threads)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == t.tobytes()


# ---------------------------------------------------------------- the decoder on malformed blobs

GUARD = 64


class Target:
    """Output arrays between guard bands, everything filled with a pattern: a refused blob must leave all of it alone."""

    def __init__(self, V, T):
        self.v = np.full(2 * GUARD + 3 * V, 0xDEADBEEF, np.uint32)
        self.t = np.full(2 * GUARD + 3 * T, 0xFEEDF00D, np.uint32)
        self.v0, self.t0 = self.v.copy(), self.t.copy()

    def decode(self, words, threads=3):
        from mlsgpu_amd import binding as bd
        raw = np.frombuffer(words.tobytes() if isinstance(words, np.ndarray) else words, np.uint8).copy()      # exactly these bytes
        rc = bd.lib().mlsgpu_hip_compact_decode(raw.ctypes.data, raw.nbytes, self.v.ctypes.data + 4 * GUARD, self.t.ctypes.data + 4 * GUARD,
                                                threads)
        st = bd.CompactStats()
        assert bd.lib().mlsgpu_hip_compact_info(raw.ctypes.data, raw.nbytes, C.byref(st)) == rc
        return rc

    def untouched(self):
        return self.v.tobytes() == self.v0.tobytes() and self.t.tobytes() == self.t0.tobytes()

    def refused(self, words):
        rc = self.decode(words)
        return rc == FORMAT and self.untouched()


def small_blob():
    """10 vertices at 16 bits, 70 triangles in two groups with exceptions in both: a few hundred bytes."""
    v = cc.ring_vertices(10, 3, offset=(1.5, 1.5, 1.5), scale=0.25)            # every coordinate in [1.25, 1.75]: lo, hi > 0
    t = cc.local_triangles(70, 10, spread=2, far=0.0, seed=2) + np.uint32(100)     # every base > 0: an exception can wrap
    t[3, 1] = t[20, 0] = t[66, 2] = 5000
    blob, st = cc.encode(v, t, 16)
    assert 200 < blob.nbytes < 600 and st["groups"] == 2 and st["exceptions"] == 3
    return v, t, blob


def test_the_small_blob_decodes():
    v, t, blob = small_blob()
    target = Target(len(v), len(t))
    assert target.decode(blob) == 0
    assert target.t[GUARD:-GUARD].tobytes() == t.tobytes()
    cc.check_vertices(target.v[GUARD:-GUARD].view(np.float32).reshape(-1, 3), v, 16)
    for arr, ref in ((target.v, target.v0), (target.t, target.t0)):
        assert arr[:GUARD].tobytes() == ref[:GUARD].tobytes() and arr[-GUARD:].tobytes() == ref[-GUARD:].tobytes()


def test_truncated_at_every_length():
    v, t, blob = small_blob()
    target = Target(len(v), len(t))
    raw = blob.tobytes()
    for n in range(len(raw)):
        assert target.refused(raw[:n]), n
    assert target.refused(raw + b"\0\0\0\0")                                    # and a word too many


def test_every_header_word_corrupted():
    """A header word that still describes a well-formed blob cannot be told from the original (a finite lo <= hi, say), so the
    corruptions are ones that cannot: a flipped top bit and all bits inverted for the counts, non-finite and swapped extents."""
    v, t, blob = small_blob()
    target = Target(len(v), len(t))
    for k in list(range(0, 8)) + [14, 15]:
        old = int(blob[k])
        for bad in (old ^ 0x80000000, old ^ 0xFFFFFFFF, old + 1 if k not in (4, 6) else old ^ 0xFFFFFFFF):
            w = blob.copy()
            w[k] = bad
            assert target.refused(w), (k, hex(int(bad)))
    for k in range(8, 14):
        for bad in (int(blob[k]) | 0x7F800000, 0x7FC00000, 0xFF800000):
            w = blob.copy()
            w[k] = bad
            assert target.refused(w), (k, hex(int(bad)))
    for a in range(3):                                                          # hi below lo
        w = blob.copy()
        w[8 + a], w[11 + a] = blob[11 + a], blob[8 + a]
        assert blob[8 + a] != blob[11 + a] and target.refused(w), a
    w32, _ = cc.encode(v, t, 32)                                                # extents at 32 bits must be zero
    w32[9] = 1
    assert target.refused(w32)


def test_every_offset_corrupted():
    v, t, blob = small_blob()
    target = Target(len(v), len(t))
    _, G, offsets_at, _ = cc.layout(blob)
    for g in range(G + 1):
        old = int(blob[offsets_at + g])
        for bad in ((old + 1) & 0xFFFFFFFF, (old - 1) & 0xFFFFFFFF, old ^ 0x80000000, 0xFFFFFFFF, int(blob[offsets_at + (g + 1) % (G + 1)])):
            w = blob.copy()
            w[offsets_at + g] = bad
            assert target.refused(w), (g, int(bad))


def test_records_corrupted():
    v, t, blob = small_blob()
    target = Target(len(v), len(t))
    _, G, offsets_at, records_at = cc.layout(blob)
    for g in range(G):
        at = records_at + int(blob[offsets_at + g])
        n = min(64, len(t) - 64 * g)
        w_g, exc = int(blob[at + 1]) & 0xFF, int(blob[at + 1]) >> 8
        assert 1 <= w_g < 32 and exc >= 1
        words = (3 * n * w_g + 31) // 32

        def with_meta(meta):
            w = blob.copy()
            w[at + 1] = meta
            return w

        assert target.refused(with_meta(0 | exc << 8))                         # w = 0
        assert target.refused(with_meta(33 | exc << 8))                        # w = 33
        assert target.refused(with_meta(255 | exc << 8))
        assert target.refused(with_meta(w_g | (3 * n + 1) << 8))                # exceptions > slots
        assert target.refused(with_meta(w_g | (exc + 1) << 8))                  # the record's length no longer fits
        assert target.refused(with_meta(32))                                   # w = 32 has no escapes and another length
        # the escapes among the slots against the exceptions, the record's length left alone
        slots = cc.unpack_bits(blob[at + 2:at + 2 + words], 3 * n, w_g)
        escape = 2 ** w_g - 1
        assert int(np.count_nonzero(slots == escape)) == exc
        one_more = slots.copy()
        one_more[np.flatnonzero(slots != escape)[0]] = escape
        one_less = slots.copy()
        one_less[np.flatnonzero(slots == escape)[-1]] = 0
        for changed in (one_more, one_less):
            w = blob.copy()
            w[at + 2:at + 2 + words] = cc.pack_bits(changed, w_g)
            assert target.refused(w)
        w = blob.copy()                                                         # base + v wraps
        w[at] = 0xFFFFFFFF
        assert target.refused(w)
        w = blob.copy()                                                         # base + an exception wraps
        w[at + 2 + words] = 0xFFFFFFFF - int(blob[at]) + 1
        assert target.refused(w)
    # a w = 32 record that claims exceptions, its length made to fit
    t32 = cc.hand_cases()[-1][1]
    blob32, _ = cc.encode(np.zeros((0, 3), np.float32), t32, 32)
    target32 = Target(0, len(t32))
    assert target32.decode(blob32) == 0 and target32.t[GUARD:-GUARD].tobytes() == t32.tobytes()
    target32 = Target(0, len(t32))
    _, _, offsets_at, records_at = cc.layout(blob32)
    w = np.concatenate([blob32, np.zeros(1, np.uint32)])
    w[records_at + 1] = 32 | 1 << 8
    w[offsets_at + 1] += 1
    w[14] += 1
    assert target32.refused(w)


def test_random_damage_never_escapes_the_buffers():
    """Whatever a damaged blob decodes to: refused with nothing written, or accepted -- a flipped bit of a slot is another
    well-formed blob -- with the sizes that the info call names and nothing written outside them."""
    from mlsgpu_amd import binding as bd
    v, t, blob = small_blob()
    rng = np.random.default_rng(11)
    refused = 0
    for _ in range(300):
        w = blob.copy()
        for k in rng.integers(0, len(w), rng.integers(1, 4)):
            w[k] = int(rng.integers(0, 2 ** 32)) if rng.random() < 0.5 else int(w[k]) ^ 1 << int(rng.integers(0, 32))
        try:
            st = bd.compact_info(w)
        except bd.FormatError:
            refused += 1
            assert Target(len(v), len(t)).refused(w)
            continue
        target = Target(st["numVertices"], st["numTriangles"])
        assert target.decode(w) == 0
        for arr, ref in ((target.v, target.v0), (target.t, target.t0)):
            assert arr[:GUARD].tobytes() == ref[:GUARD].tobytes() and arr[-GUARD:].tobytes() == ref[-GUARD:].tobytes()
    assert 30 < refused < 300
