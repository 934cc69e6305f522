"""The triangle grid under mlsgpu_hip_mesh_deviation and mlsgpu_hip_mesh_self_intersections (mlsgpu_amd/csrc/meshgrid.hpp) on
the GPU: with timing on, the cell size the grid settled on, its records and the number of sizes it counted are exactly the
numpy model's (meshgrid_cases.plan), and the report is its oracle's as ever.

The cell size, the record count and the launch count are the implementation's plan, not part of either report's contract:
both reports are the same for every cell size, which is why no test of the reports notices a change of the grid and these
tests exist.  A later tuning change may update the model."""
import numpy as np
import pytest

import deviation_cases as dc
import intersect_cases as ic
import meshgrid_cases as mg
from gpu_common import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def timed(ctx, call):
    ctx.reset_stats()
    ctx.set_timing(True)
    try:
        return call()
    finally:
        ctx.set_timing(False)


@pytest.mark.parametrize("case", mg.intersect_cases(), ids=lambda c: c.name)
def test_self_intersections(ctx, case):
    from mlsgpu_amd import binding as b
    P = mg.plan(case.vertices, case.triangles, 0.0)
    triangles = np.asarray(case.triangles).astype(np.uint32)
    want = ic.self_intersections(case.vertices, case.triangles)
    # without the list the binding makes ONE call of the entry point: the statistics are that call's, not the sum of two
    partners, _, st = timed(ctx, lambda: b.mesh_self_intersections(ctx, case.vertices, triangles, want_pairs=False))
    figures = (ctx.stat("intersect.cellsize")[0], ctx.stat("intersect.records")[0], ctx.stat("kernel.intersect.count")[1])
    print(case.name, figures, P)
    assert figures == (P.cell_size, float(P.records), P.accepted)
    ic.assert_same((partners, None, st), want)
    ic.assert_same(b.mesh_self_intersections(ctx, case.vertices, triangles), want)


@pytest.mark.parametrize("case", mg.deviation_cases(), ids=lambda c: c.name)
def test_deviation(ctx, case):
    from mlsgpu_amd import binding as b
    P = mg.plan(case.vertices, case.triangles, case.D)
    got = timed(ctx, lambda: b.mesh_deviation(ctx, case.points, case.vertices, np.asarray(case.triangles).astype(np.uint32), case.D))
    figures = (ctx.stat("deviation.cellsize")[0], ctx.stat("deviation.pairs")[0], ctx.stat("kernel.deviation.count")[1])
    print(case.name, figures, P)
    assert figures == (P.cell_size, float(P.records), P.accepted)
    dc.assert_same(got, dc.deviation(case.points, case.vertices, case.triangles, case.D))
