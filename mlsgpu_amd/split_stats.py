"""mlsgpu_split_stats (include/mlsgpu_hip.h), the statistics of mesh_split_edges and Mesher.split_edges."""
import ctypes as C

from .binding import Stats


class SplitStats(Stats):
    """mlsgpu_split_stats: what took no part, edges, interior regular and boundary edges, rounds, splits, those of boundary
    edges, whether the last round found no candidate and whether a limit ended the rounds, the long edges before and after and
    those that cannot be split, the sizes of the result, the triangle quality and the largest squared edge length before and
    after."""
    _fields_ = [("numVertices", C.c_uint64), ("numTriangles", C.c_uint64), ("outOfRangeTriangles", C.c_uint64),
                ("degenerateTriangles", C.c_uint64), ("numEdges", C.c_uint64), ("interiorEdges", C.c_uint64),
                ("boundaryEdges", C.c_uint64), ("rounds", C.c_uint64), ("splits", C.c_uint64), ("boundarySplits", C.c_uint64),
                ("converged", C.c_uint64), ("limited", C.c_uint64), ("longBefore", C.c_uint64), ("longAfter", C.c_uint64),
                ("blockedAfter", C.c_uint64), ("outVertices", C.c_uint64), ("outTriangles", C.c_uint64),
                ("minQualityBefore", C.c_double), ("minQualityAfter", C.c_double), ("maxLengthSqBefore", C.c_double),
                ("maxLengthSqAfter", C.c_double), ("qualityBefore", C.c_uint64 * 16), ("qualityAfter", C.c_uint64 * 16)]
