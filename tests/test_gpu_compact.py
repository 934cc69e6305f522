"""The compact read-back on the device against the numpy oracle: the whole blob byte for byte."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import compact_cases as cc
import sink_cases as sk
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

BITS = (8, 16, 21, 24, 32)


def check(ctx, v, t, b):
    """Device blob == oracle blob, the statistics, and the library's decoder brings the inputs back."""
    from mlsgpu_amd import binding as bd
    want, want_st = cc.encode(v, t, b)
    got, st = bd.mesh_compact(ctx, v, t, b)
    cc.same_stats(st, want_st)
    assert got.tobytes() == want.tobytes()
    back_v, back_t = bd.compact_decode(got)
    assert back_t.tobytes() == np.ascontiguousarray(t, np.uint32).tobytes()
    cc.check_vertices(back_v, v, b)
    return st


def vertices_of(V, seed):
    """Negative coordinates, both zeros, x near 10^6, and (from 8 vertices on) a z axis with hi = lo."""
    v = cc.ring_vertices(V, seed, offset=(1.0e6, -3.0, 0.0), scale=2.0)
    if V >= 8:
        v[:, 2] = 0.25
    return v


@pytest.mark.parametrize("b", BITS)
@pytest.mark.parametrize("V,T", ((0, 0), (1, 1), (63, 63), (64, 64), (65, 65), (1000, 257), (0, 64), (64, 0)))
def test_sizes_and_bits(ctx, V, T, b):
    check(ctx, vertices_of(V, V + b), cc.local_triangles(T, max(V, 1), seed=T), b)


def test_beyond_one_tile_of_the_scan(ctx):
    """2050 groups: the offsets cross a tile (2048 elements) of the scan, the last group is partial."""
    V, T = 70000, 64 * 2049 + 1
    st = check(ctx, vertices_of(V, 1), cc.local_triangles(T, V, seed=4), 16)
    assert st["groups"] == 2050 and st["exceptions"] > 1000 and sum(1 for n in st["widthHistogram"] if n) >= 4


def test_zeros_and_flat_axes(ctx):
    v = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], np.float32)
    for b in (8, 24):
        st = check(ctx, v, np.array([[0, 1, 2]], np.uint32), b)
        assert st["step"] == [0.0, 0.0, 0.0]
    v[2] = (-5.0, 1.0e6, -1.0e6)
    check(ctx, v, np.array([[0, 1, 2]], np.uint32), 21)


@pytest.mark.parametrize("case", cc.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(ctx, case):
    name, t, nbytes, w, exc = case
    st = check(ctx, np.zeros((0, 3), np.float32), t, 32)
    assert st["blobBytes"] == nbytes and st["widthHistogram"][w] == 1 and st["exceptions"] == exc


def test_arbitrary_indices_and_bits(ctx):
    """Indices are not compared with the vertex count, and at 32 bits any float bits pass."""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 2 ** 32, (300, 3), dtype=np.uint64).astype(np.uint32)
    t[:64] = rng.integers(0, 2 ** 32, 1, dtype=np.uint64).astype(np.uint32) + rng.integers(0, 9, (64, 3)).astype(np.uint32)
    v = rng.integers(0, 2 ** 32, (7, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)
    check(ctx, v, t, 32)
    check(ctx, vertices_of(7, 0), t, 16)


def small_correct_call(ctx):
    name, t, nbytes, w, exc = cc.hand_cases()[2]
    assert check(ctx, vertices_of(9, 9), t, 16)["exceptions"] == exc


def test_nan_and_refused_arguments(ctx):
    from mlsgpu_amd import binding as bd
    v, t = vertices_of(100, 3), cc.local_triangles(70, 100)
    v[7, 2] = np.nan
    v[50, 0] = -np.inf
    for b in (8, 16, 24):
        with pytest.raises(bd.InvalidArgument, match="2 vertex coordinates are not finite"):
            bd.mesh_compact(ctx, v, t, b)
        small_correct_call(ctx)
    check(ctx, v, t, 32)                                                        # bits are bits
    for b in (0, 7, 25, 31, 33):
        with pytest.raises(bd.InvalidArgument):
            bd.mesh_compact(ctx, vertices_of(10, 1), t, b)
    one = bd.DeviceBuffer(ctx, array=np.zeros(3, np.uint32))
    st = bd.CompactStats()
    for n_vertices, n_triangles in ((2 ** 32, 1), (1, (2 ** 32 + 2) // 3), (1, 64 * ((2 ** 32) // 194 + 1))):
        with pytest.raises(bd.LengthError):             # refused before anything is allocated or launched: the buffer holds 12 bytes
            bd.check(bd.lib().mlsgpu_hip_mesh_compact(ctx.h, one.ptr, n_vertices, one.ptr, n_triangles, 32, None, 0, C.byref(st)))
        small_correct_call(ctx)
    with pytest.raises(bd.InvalidArgument):              # a misaligned output
        bd.check(bd.lib().mlsgpu_hip_mesh_compact(ctx.h, one.ptr, 1, one.ptr, 1, 32, one.ptr + 2, 1000, C.byref(st)))
    one.free()


def test_capacity_rule_and_guard_bands(ctx):
    from mlsgpu_amd import binding as bd
    v, t = vertices_of(300, 2), cc.local_triangles(200, 300, seed=8)
    want, want_st = cc.encode(v, t, 16)
    n, G = len(want), 256
    dv, dt = bd.DeviceBuffer(ctx, array=v), bd.DeviceBuffer(ctx, array=t)
    band = np.full(2 * G + n, 0xDEADBEEF, np.uint32)
    out = bd.DeviceBuffer(ctx, array=band)

    def call(ptr, capacity):
        st = bd.CompactStats()
        rc = bd.lib().mlsgpu_hip_mesh_compact(ctx.h, dv.ptr, len(v), dt.ptr, len(t), 16, ptr, capacity, C.byref(st))
        return rc, st.as_dict()

    for ptr, capacity in ((None, 0), (None, 10 ** 9), (out.ptr + 4 * G, 0), (out.ptr + 4 * G, 4 * n - 1)):
        rc, st = call(ptr, capacity)
        with pytest.raises(bd.LengthError):
            bd.check(rc)
        cc.same_stats(st, want_st)                                              # the planning pass alone: complete
        assert out.download(np.uint32).tobytes() == band.tobytes()             # and nothing written
    for capacity in (4 * n, 4 * n + 4 * G):                                     # exact, and more than enough
        out.upload(band)
        rc, st = call(out.ptr + 4 * G, capacity)
        assert rc == 0
        cc.same_stats(st, want_st)
        got = out.download(np.uint32)
        assert got[:G].tobytes() == band[:G].tobytes() and got[G + n:].tobytes() == band[G + n:].tobytes()
        assert got[G:G + n].tobytes() == want.tobytes()
    assert dv.download(np.float32).tobytes() == v.tobytes() and dt.download(np.uint32).tobytes() == t.tobytes()
    for buf in (dv, dt, out):
        buf.free()


# ---------------------------------------------------------------- the device sink

def test_sink(ctx, tmp_path):
    """A sheet in two chunks: every chunk's blob is the oracle's of the downloaded chunk, decodes to it, and nothing changes."""
    from mlsgpu_amd import binding as bd
    from test_gpu_deviation import filled, state_of
    meshes = sk.tiled_sheet(21, 48, 48, 8, 0.15, 0.3, 2)
    sink = filled(ctx, meshes)
    with pytest.raises(bd.InvalidArgument):
        sink.chunk_compact(0)                                                   # before finalize
    assert sink.finalize() == 2
    pinned = bd.PinnedBuffer(1 << 20)

    def against_the_download():
        before = state_of(sink, 2, tmp_path)
        triangles = 0
        for i in range(2):
            c = sink.chunk(i)
            assert len(c["triangles"]) > 100
            triangles += len(c["triangles"])
            for b in (32, 16):
                want, want_st = cc.encode(c["vertices"], c["triangles"], b)
                blob, st = sink.chunk_compact(i, b)
                cc.same_stats(st, want_st)
                assert blob.tobytes() == want.tobytes()
                v, t = bd.compact_decode(blob)
                assert t.tobytes() == c["triangles"].tobytes()                  # lossless
                cc.check_vertices(v, c["vertices"], b)                          # exact at 32, within the bound at 16
                view, st = sink.chunk_compact(i, b, out=pinned)                 # into pinned memory: the same bytes
                assert view.tobytes() == want.tobytes()
            st = bd.CompactStats()
            small = np.full(16, 0xDEADBEEF, np.uint32)
            rc = bd.lib().mlsgpu_hip_mesher_chunk_compact(sink.h, i, 16, small.ctypes.data, small.nbytes, C.byref(st))
            with pytest.raises(bd.LengthError):
                bd.check(rc)
            assert (small == 0xDEADBEEF).all() and st.blobBytes == want_st["blobBytes"]
        with pytest.raises(bd.InvalidArgument):
            sink.chunk_compact(2)
        with pytest.raises(bd.InvalidArgument):
            sink.chunk_compact(0, 7)
        assert state_of(sink, 2, tmp_path) == before
        return triangles

    n = against_the_download()
    sink.simplify((-1.0, -1.0, -1.0), 3.0)
    assert against_the_download() < n
    pinned.free()
    sink.close()


# ---------------------------------------------------------------- reconstruct --compact

def test_reconstruct_compact(ctx, tmp_path):
    """examples/reconstruct --compact: with 32 the same file and one more line; with 16 the same triangles.  Behind --simplify,
    whose output does not depend on the order in which the farm's threads delivered the blocks."""
    from test_gpu_simplify import shells
    from test_host_cpp import build_example
    from mlsgpu_amd import synth
    exe = build_example(tmp_path, "reconstruct")
    cloud = shells()
    rows = np.zeros(len(cloud), synth.PLY_ROW)
    rows["p"], rows["n"], rows["r"] = cloud["position"], cloud["normal"], cloud["radius"]
    (tmp_path / "in.ply").write_bytes(synth.ply_header(len(rows)) + rows.tobytes())

    def run(flags, out):
        cmd = [exe, "--weld", "device", "--simplify", "4"] + flags + [str(tmp_path / "in.ply"), str(tmp_path / out), "1.0", "1.5", "4", "3", "0.02", "8000"]
        return subprocess.check_output(cmd, timeout=300).decode().splitlines()

    plain = run([], "plain.ply")
    pattern = r"compact bits (\d+) raw (\d+) blob (\d+) ratio ([0-9.]+) exceptions (\d+) step (\S+) (\S+) (\S+)"
    sizes = {}
    for bits in (32, 16):
        lines = run(["--compact", str(bits)], "c%d.ply" % bits)
        assert len(lines) == len(plain) + 1 and lines[:-1] == plain, lines
        m = re.fullmatch(pattern, lines[-1])
        assert m and int(m.group(1)) == bits, lines[-1]
        raw, blob = int(m.group(2)), int(m.group(3))
        assert raw > 12 * 200 and blob < raw and abs(float(m.group(4)) - blob / raw) < 1e-4
        assert all((float(x) == 0.0) == (bits == 32) for x in m.groups()[5:])
        sizes[bits] = blob
    assert sizes[16] < sizes[32]
    want = (tmp_path / "plain.ply").read_bytes()
    assert (tmp_path / "c32.ply").read_bytes() == want
    got = (tmp_path / "c16.ply").read_bytes()
    head = want.index(b"end_header\n") + len(b"end_header\n")
    assert len(got) == len(want) and got[:head] == want[:head]
    nv = int(re.search(rb"element vertex (\d+)", want).group(1))
    assert got[head + 12 * nv:] == want[head + 12 * nv:]                       # the faces, bit for bit
    a = np.frombuffer(got[head:head + 12 * nv], np.float32).reshape(-1, 3)
    cc.check_vertices(a, np.frombuffer(want[head:head + 12 * nv], np.float32).reshape(-1, 3), 16)
    for flags, why in ((["--weld", "host", "--compact", "16"], b"--compact needs --weld device"), (["--compact", "5"], b"--compact takes")):
        refused = subprocess.run([exe, "--weld", "device"] + flags + [str(tmp_path / "in.ply"), str(tmp_path / "no.ply"), "1.0"],
                                 capture_output=True, timeout=300)
        assert refused.returncode != 0 and why in refused.stderr
        assert not (tmp_path / "no.ply").exists()
