"""The preconditions of tests/test_gpu_meshgrid.py, checked with the numpy model of the grid's plan (meshgrid_cases) alone: every
case really takes the path it is named for -- sizes refused by the cell cap, several accepted sizes, one cell in all.

The model's figures are the implementation's plan, not part of the deviation or the self-intersection report's contract; a
later tuning change may update the model, and these expectations with it."""
import numpy as np
import pytest

import meshgrid_cases as mg


@pytest.mark.parametrize("case", mg.intersect_cases(), ids=lambda c: c.name)
def test_intersect_cases_take_their_paths(case):
    P = mg.plan(case.vertices, case.triangles, 0.0)
    assert P.live >= 2                                  # below that the report lays no grid
    mg.check_path(case, P)


@pytest.mark.parametrize("case", mg.deviation_cases(), ids=lambda c: c.name)
def test_deviation_cases_take_their_paths(case):
    assert len(case.points) > 0 and case.D == float(np.float32(case.D)) > 0.0
    mg.check_path(case, mg.plan(case.vertices, case.triangles, case.D))


def test_the_paths_between_them():
    names = {c.path for c in mg.intersect_cases() + mg.deviation_cases()}
    assert names == {"several cells", "doubled", "refused", "side", "one cell", "mean extent", "twice D"}
    refused = [mg.plan(c.vertices, c.triangles, c.D).refused for c in mg.intersect_cases() + mg.deviation_cases() if c.path == "refused"]
    assert refused == [2, 2]


def test_model_by_hand():
    """Two triangles in the unit square's plane and one far off, worked out on paper: side 8, eSide 4 (8 < 16), extents 1, 1
    and 2 in units of 2^-20 * 16, mean 4 / 3, box [0, 8] x [0, 2] x [0, 0]: 7 x 2 x 1 cells of 4 / 3."""
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [6, 0, 0], [8, 0, 0], [8, 2, 0]])
    t = [[0, 1, 2], [1, 3, 2], [4, 5, 6], [7, 0, 1], [2, 2, 3]]            # the last two take no part
    P = mg.plan(v, t)
    assert (P.live, P.side, P.e_side, P.extent_sum) == (3, 8.0, 4, (1 + 1 + 2) << 16)
    assert P.first_size == 4.0 / 3.0 * 1.0 and P.n == [7, 2, 1] and P.key_bits == 4
    # cells: [0, 1] -> 0 .. 0; [6, 8] -> 4 .. 6; y [0, 1] -> 0 .. 0, [0, 2] -> 0 .. 1
    assert (P.records, P.accepted, P.refused) == (1 + 1 + 3 * 2, 1, 0)
    Q = mg.plan(v, t, 2.0)                              # D = 2: the first cell is 4, the box [-2, 10] x [-2, 4] x [-2, 2]
    # x [-2, 3] -> 0 .. 1 and [4, 10] -> 1 .. 3; y [-2, 3] and [-2, 4] -> 0 .. 1; z [-2, 2] -> 0 .. 1
    assert Q.first_size == 4.0 and Q.n == [4, 2, 2] and Q.records == 2 * (2 * 2 * 2) + 3 * 2 * 2
