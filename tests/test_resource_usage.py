"""*_resource_usage returns what *_create allocates: both walk one buffer list (loads the library only, no GPU).

The figures are the sums of the sizes mlsgpu_hip_tree_create / mlsgpu_hip_marching_create hand to hipMalloc (device memory
only: the pinned read-backs and the mailboxes are not counted).  A change that resizes a buffer updates them knowingly."""
import ctypes as C

import pytest

CELL_BYTES = 872        # MLSGPU_MARCHING_MAX_CELL_BYTES


@pytest.mark.parametrize("levels,splats,expect", [(4, 1000, 196404), (6, 100000, 18608528)])
def test_tree_resource_usage(levels, splats, expect):
    import mlsgpu_amd
    assert mlsgpu_amd.lib().mlsgpu_hip_tree_resource_usage(levels, splats) == expect


MARCHING = [
    # width, height, depth, swathe, mesh memory, alignment, bytes
    (33, 33, 32, 32, 32 * 32 * 2 * CELL_BYTES, (8, 8, 8), 1897984),
    (20, 18, 24, 8, 19 * 17 * 3 * CELL_BYTES, (1, 1, 1), 1084964),              # several swathes: the sort-weld buffers too
    (256, 256, 256, 256, 255 * 255 * 2 * CELL_BYTES, (8, 8, 8), 443403708),     # the worker's default lane
]


@pytest.mark.parametrize("w,h,d,swathe,mesh,align,expect", MARCHING)
def test_marching_resource_usage(w, h, d, swathe, mesh, align, expect):
    import mlsgpu_amd
    alignment = (C.c_uint32 * 3)(*align)
    assert mlsgpu_amd.lib().mlsgpu_hip_marching_resource_usage(w, h, d, swathe, mesh, alignment) == expect


def test_worker_resource_usage_is_the_lane():
    import mlsgpu_amd
    from mlsgpu_amd.binding import WorkerConfig
    L = mlsgpu_amd.lib()
    cfg = WorkerConfig()
    cfg.maxBucketSplats = 100000
    lane = 443403708 + 18608528
    assert lane == 462012236
    assert L.mlsgpu_hip_worker_resource_usage(C.byref(cfg)) == lane
    assert L.mlsgpu_hip_worker_resource_usage_lanes(C.byref(cfg), 3) == 3 * lane
