"""The kernels against the float64 references of tests/fp64_reference.py, next to bit parity with the oracle: the MLS field
at four octree settings with every kernel variant, marching on the special-value fields with both welds and both triangle
routes, and the whole worker at non-default (levels, subsampling)."""
import numpy as np
import pytest

import fp64_reference as fr
import oracle_binding as ob
from gpu_common import assert_batches_equal, ctx  # noqa: F401
from test_fp64_oracle import (CLOSED, MLS_CLOUDS, TREES, at, check_field, check_mesh, cloud_and_sums, march_field,
                              oracle_field)
from test_oracle_marching import host_generator

pytestmark = pytest.mark.gpu

GPU_LIMITS = [0.5, 1.0, 3.0]


def _same_field(got, exp, what):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=str(what))
    ok = ~np.isnan(exp)
    np.testing.assert_array_equal(got[ok].view(np.uint32), exp[ok].view(np.uint32), err_msg=str(what))


@pytest.mark.parametrize("name", MLS_CLOUDS)
def test_gpu_mls_field_vs_fp64(ctx, name):
    """SplatTree + MlsFunctor.set (as the worker runs them) at four (levels, subsampling), kernels 1 / 4 / 5, both shapes,
    three boundary limits: bit-equal to the oracle and within the measured tolerances of the fp64 field.  The raw-radius
    path (a non-mutating build) gives the same bits as the mutated one."""
    import mlsgpu_amd as m
    cloud, size, offset, corners, s = cloud_and_sums(name)
    W8, H8, D8 = [(x + 7) // 8 * 8 for x in size]
    rows = H8 * D8
    sw = m.Swathe(size[0], size[1], H8, 0, 0, size[2] - 1)
    dfield = m.DeviceBuffer(ctx, array=np.full((rows, W8), -7.0, np.float32))
    for levels, sub in TREES:
        buf = m.DeviceBuffer(ctx, array=cloud)
        tree = m.SplatTree(ctx, levels, len(cloud))
        tree.enqueue_build(buf, 0, len(cloud), size, offset, sub)
        raw_buf = m.DeviceBuffer(ctx, array=cloud)
        raw_tree = m.SplatTree(ctx, levels, len(cloud))
        raw_tree.set_mutate(False)
        raw_tree.enqueue_build(raw_buf, 0, len(cloud), size, offset, sub)
        ctx.synchronize()
        mutated = cloud.copy()
        t = ob.Tree(mutated, 0, len(mutated), size, offset, sub, levels)
        np.testing.assert_array_equal(buf.download(m.SPLAT_DTYPE, len(cloud)).view(np.uint32), mutated.view(np.uint32))
        for shape in (0, 1):
            for limit in GPU_LIMITS:
                exp, _ = oracle_field(mutated, t.commands, t.start, size, offset, sub, shape, limit)
                check_field(at(exp, H8, corners), s, shape, limit, (name, levels, sub, shape, limit))
                for variant in (1, 4, 5):
                    what = (name, levels, sub, shape, limit, variant)
                    for tr in ((tree, raw_tree) if limit == 1.0 else (tree,)):
                        gen = m.MlsFunctor(ctx, shape)
                        gen.set(offset, tr, sub)
                        gen.set_boundary_limit(limit)
                        gen.set_variant(variant)
                        dfield.upload(np.full((rows, W8), -7.0, np.float32))
                        gen.enqueue(dfield, W8, rows, sw)
                        ctx.synchronize()
                        got = dfield.download(np.float32).reshape(rows, W8)
                        _same_field(got, exp, what + (tr is raw_tree,))
                        check_field(at(got, H8, corners), s, shape, limit, what)
        np.testing.assert_array_equal(raw_buf.download(m.SPLAT_DTYPE, len(cloud)).view(np.uint32), cloud.view(np.uint32))
        del tree, raw_tree, buf, raw_buf


def _canon_nan(batches):
    """Batches with every NaN vertex coordinate made one bit pattern: IEEE leaves the sign and payload of the NaN that
    inf * 0 makes to the platform; WHERE the NaNs are is still compared exactly."""
    out = []
    for b in batches:
        b = dict(b)
        v = b["vertices"].copy()
        v[np.isnan(v)] = np.float32(np.nan)
        b["vertices"] = v
        out.append(b)
    return out


GPU_MARCH_CASES = ["torus", "sphere"] + ["special_" + k for k in ("zeros", "denormals", "flt_max", "nonfinite", "mixed")]


@pytest.mark.parametrize("name", GPU_MARCH_CASES)
def test_gpu_marching_vs_fp64(ctx, name, monkeypatch):
    """Marching on the torus, a sphere and the special-value fields (+-0, denormals, FLT_MAX neighbours, +-inf, NaN of
    both signs), with the lattice and the sort weld, both triangle routes, ample and two slices of mesh memory: batches and
    counters equal the oracle's, and the mesh equals marching_fp64 (edges, triangle count, positions, the float32 formula
    on flagged edges, Euler characteristic and orientation of the closed surfaces)."""
    import mlsgpu_amd as m
    field = march_field(name)
    ref = fr.marching_fp64(field)
    D, H, W = field.shape
    size = (W, H, D)
    mw, mh, md = W + 3, H + 2, 72           # maxSwathe 64 < maxDepth 72 keeps the sort weld's buffers allocated
    alignment = (8, 8, 8)

    def fn(xs, ys, z):
        return field[z]
    for weld in ("lattice", "sort"):
        if weld == "sort":
            monkeypatch.setenv("MLSGPU_HIP_WELD", "sort")
        else:
            monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
        for route in ("0", "1"):
            monkeypatch.setenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", route)
            for slices in (400, 2):
                mesh_memory = (mw - 1) * (mh - 1) * 872 * slices
                what = (name, weld, route, slices)
                mc = m.Marching(ctx, mw, mh, md, 64, mesh_memory, alignment)
                got = mc.generate(m.binding.HostGenerator(ctx, fn, alignment), size)
                oracle = ob.MarchingOracle(mw, mh, md, 64, mesh_memory, alignment)
                exp = oracle.generate(host_generator(lambda x, y, z: field[z]), size)
                for g, e in zip(got, exp):
                    np.testing.assert_array_equal(np.isnan(g["vertices"]), np.isnan(e["vertices"]), err_msg=str(what))
                assert_batches_equal(_canon_nan(got), _canon_nan(exp))
                st, cnt = oracle.stats(), mc.counters()
                for k in ("shipouts", "overflows", "occupied", "unwelded", "indices", "welded", "external"):
                    assert st[k] == cnt[k], (what, k)
                c = check_mesh(got, ref, name)
                if name in CLOSED:
                    assert c["euler"] == CLOSED[name]
                del mc
    monkeypatch.delenv("MLSGPU_HIP_WELD", raising=False)
    monkeypatch.delenv("MLSGPU_HIP_TRIANGLES_BY_CELLS", raising=False)


# ---- the whole worker at non-default (levels, subsampling) ---------------------------------------------------------------

WORKER_PAIRS = [(4, 3), (5, 4), (3, 5), (7, 3)]


def worker_buckets():
    """Three buckets (splats, low extent, numVertices): a sphere at the origin, a shifted sphere at a low extent that is not
    a multiple of 8 (the worker takes lowExtent >= 0) and a shells cloud; numVertices within the smallest capacity below (64
    per side) and none a multiple of 8."""
    from mlsgpu_amd import synth
    a = synth.sphere_cloud(6000, (30.5, 28.0, 26.25), 20.0, 1.0, 2.0, 21)
    b = synth.sphere_cloud(5000, (12.0, 14.5, 11.0), 9.0, 1.0, 2.5, 22)
    b["position"] += np.array([23, 7, 41], np.float32)
    c = synth.shells_cloud(7000, 50.0, 7.0, 1.0, 2.0, 23)
    return [(a, (0, 0, 0), (61, 59, 57)), (b, (23, 7, 41), (29, 31, 27)), (c, (0, 0, 0), (51, 50, 49))]


@pytest.mark.parametrize("levels,sub", WORKER_PAIRS)
def test_worker_non_default_tree(ctx, levels, sub):
    """Worker.process and Worker.process_batch (three lanes) with max_cells the largest the pair allows: every bucket's
    batches bit-equal to the oracle's bucket at the same levels / subsampling."""
    import mlsgpu_amd as m
    max_cells = (1 << (levels + sub - 1)) - 1
    swathe = (max_cells + 1 + 7) // 8 * 8
    mesh_memory = max_cells * max_cells * 2 * 872
    buckets = worker_buckets()
    exps = []
    for cloud, low, nv in buckets:
        exp, st = ob.bucket(cloud.copy(), 0, len(cloud), nv, low, levels=levels, subsampling=sub, max_cells=max_cells,
                            max_swathe=swathe, mesh_memory=mesh_memory)
        assert st["welded"] > 0
        exps.append(exp)
    total = sum(len(c) for c, _, _ in buckets)
    w = m.Worker(ctx, total, max_cells=max_cells, levels=levels, subsampling=sub)
    for (cloud, low, nv), exp in zip(buckets, exps):
        buf = m.DeviceBuffer(ctx, array=cloud)
        assert_batches_equal(w.process(buf, 0, len(cloud), low, nv), exp)
        del buf
    allc = np.concatenate([c for c, _, _ in buckets])
    items, first = [], 0
    for cloud, low, nv in buckets:
        items.append((first, len(cloud), low, nv))
        first += len(cloud)
    w.set_batch(3)
    buf = m.DeviceBuffer(ctx, array=allc)
    got = w.process_batch(buf, items)
    assert len(got) == 3
    for g, exp in zip(got, exps):
        assert_batches_equal(g, exp)
    del w, buf
