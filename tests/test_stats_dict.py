"""as_dict() of every statistics structure of the binding: the keys, their order and the kind of every value, written down
as they have been since each structure came.  The sink tests compare these dicts with == against the oracles', whose values
are ints, floats and lists, so a kind matters as much as a name.  Needs no GPU and does not load the library."""
import pytest

from mlsgpu_amd import binding as b

INTS16, INTS33, FLOATS3 = ("list", int, 16), ("list", int, 33), ("list", float, 3)

# per structure: (names, kind) runs in order; a kind is int, float or ("list", element type, length)
SHAPES = {
    "SimplifyStats": [("inVertices inTriangles outVertices outTriangles collapsedTriangles duplicateTriangles", int)],
    "SimplifyQuadricStats": [("inVertices inTriangles outVertices outTriangles collapsedTriangles duplicateTriangles "
                              "solvedVertices flatVertices escapedVertices scaleExponent", int)],
    "NormalsStats": [("numVertices numTriangles outOfRangeTriangles nonFiniteTriangles zeroNormals scaleExponent", int)],
    "SmoothStats": [("numVertices numTriangles outOfRangeTriangles degenerateTriangles numEdges boundaryEdges boundaryVertices "
                     "isolatedVertices passes scaleExponent", int),
                    ("maxMove maxCoordinate", float)],
    "FlipStats": [("numVertices numTriangles outOfRangeTriangles degenerateTriangles numEdges interiorEdges rounds flips converged "
                   "nonDelaunayBefore nonDelaunayAfter blockedAfter", int),
                  ("minQualityBefore minQualityAfter", float),
                  ("qualityBefore qualityAfter", INTS16)],
    "CollapseStats": [("numVertices numTriangles outOfRangeTriangles degenerateTriangles numEdges interiorEdges fixedVertices rounds "
                       "collapses converged shortBefore shortAfter blockedAfter unusedVertices outVertices outTriangles", int),
                      ("minQualityBefore minQualityAfter minLengthSqBefore minLengthSqAfter", float),
                      ("qualityBefore qualityAfter", INTS16)],
    "FillStats": [("numVertices numTriangles outOfRangeTriangles degenerateTriangles boundaryEdges irregularEdges loops filledLoops "
                   "longLoops pinnedLoops filledEdges longestLoop outVertices outTriangles scaleExponent", int)],
    "Deviation": [("numPoints numVertices numTriangles outOfRangeTriangles degenerateTriangles within beyond farthestPoint "
                   "farthestChunk", int),
                  ("histogram", INTS16),
                  ("sumQ scaleExponent", int),
                  ("maxDistance2 limit2 meanSquare", float)],
    "SelfIntersections": [("numVertices numTriangles outOfRangeTriangles degenerateTriangles candidatePairs crossingPairs "
                           "crossingTriangles lowestA lowestB maxPartners maxPartnersTriangle lowestChunk crossingChunks", int)],
    "CompactStats": [("numVertices numTriangles vertexBits blobBytes vertexBytes triangleBytes groups exceptions", int),
                     ("widthHistogram", INTS33),
                     ("step", FLOATS3)],
    "RepairStats": [("numVertices numTriangles outOfRangeTriangles degenerateTriangles repeatedSides droppedTriangles unusedVertices "
                     "splitVertices addedVertices outVertices outTriangles", int)],
}


def kind_of(value):
    if type(value) is list:
        kinds = set(type(x) for x in value)
        assert len(kinds) == 1, kinds
        return ("list", kinds.pop(), len(value))
    return type(value)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_as_dict_of_a_zeroed_structure(name):
    got = getattr(b, name)().as_dict()
    want = [(key, kind) for names, kind in SHAPES[name] for key in names.split()]
    assert [(key, kind_of(value)) for key, value in got.items()] == want
    assert all(v == 0 if type(v) is not list else v == [0] * len(v) for v in got.values())


def test_every_stats_structure_is_listed():
    """A structure with an as_dict that this file does not know fails here, so that it gets a row above."""
    import ctypes as C
    found = sorted(name for name, cls in vars(b).items()
                   if isinstance(cls, type) and issubclass(cls, C.Structure) and hasattr(cls, "as_dict") and hasattr(cls, "_fields_"))
    assert found == sorted(SHAPES)


def test_values_come_through():
    """Not only zeros: a negative exponent, a double, an element of each kind of array, and Deviation's derived mean."""
    st = b.CompactStats(numVertices=2 ** 40, step=(0.5, 0.25, 0.125))
    st.widthHistogram[32] = 7
    d = st.as_dict()
    assert d["numVertices"] == 2 ** 40 and d["step"] == [0.5, 0.25, 0.125] and d["widthHistogram"][32] == 7
    d = b.Deviation(within=4, sumQ=3 << 30, scaleExponent=-2, maxDistance2=1.5).as_dict()
    assert (d["scaleExponent"], d["maxDistance2"], d["meanSquare"]) == (-2, 1.5, 3 * 0.25 / 4) and list(d)[-1] == "meanSquare"
    assert b.SmoothStats(scaleExponent=-7, maxMove=0.125).as_dict()["scaleExponent"] == -7
