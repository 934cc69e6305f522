"""mlsgpu_amd -- MI355X (gfx950) implementation of mlsgpu's per-bucket device pipeline.

The product is the HIP library ``libmlsgpu_hip.so`` (C-ABI: include/mlsgpu_hip.h) and the C++
classes in ``mlsgpu_amd/host`` that mirror the reference's call surface.  This Python package is
a thin ctypes binding of the same C-ABI, used by the tests and by bench.py.  There is no CPU
fallback: importing :mod:`mlsgpu_amd.binding` without the built library raises.
"""
from .binding import (BucketFarm, CollapseStats, CompactStats, Context, DensityError, Deviation, DeviceBuffer, FillStats, FlipStats, FormatError, HipError, HostMesher, InvalidArgument, LengthError, Marching, Mesher, MlsError,
                      MlsFunctor, NormalsStats, REPAIR_SPLIT_PINCHES, RepairStats, SPLAT_DTYPE, SelfIntersections, SimplifyQuadricStats, SimplifyStats, SmoothStats, SplatTree, Swathe, Topology, Worker, WorkerConfig, lib, library_path, compact_decode, compact_info, mesh_collapse_edges, mesh_compact, mesh_deviation, mesh_fill_holes, mesh_flip_edges,
                      mesh_normals, mesh_repair, mesh_self_intersections, mesh_simplify, mesh_simplify_quadric, mesh_smooth, mesh_split_edges, mesh_topology, mesher_deviation, mesher_fill_holes, mesher_repair, mesher_self_intersections)
from .split_stats import SplitStats

__all__ = ["BucketFarm", "CollapseStats", "CompactStats", "Context", "DensityError", "Deviation", "DeviceBuffer", "FillStats", "FlipStats", "FormatError", "HipError", "HostMesher", "InvalidArgument", "LengthError", "Marching", "Mesher", "MlsError",
           "MlsFunctor", "NormalsStats", "REPAIR_SPLIT_PINCHES", "RepairStats", "SPLAT_DTYPE", "SelfIntersections", "SimplifyQuadricStats", "SimplifyStats", "SmoothStats", "SplatTree", "SplitStats", "Swathe", "Topology", "Worker", "WorkerConfig", "lib", "library_path", "compact_decode", "compact_info", "mesh_collapse_edges", "mesh_compact", "mesh_deviation", "mesh_fill_holes", "mesh_flip_edges",
           "mesh_normals", "mesh_repair", "mesh_self_intersections", "mesh_simplify", "mesh_simplify_quadric", "mesh_smooth", "mesh_split_edges", "mesh_topology", "mesher_deviation", "mesher_fill_holes", "mesher_repair", "mesher_self_intersections"]
