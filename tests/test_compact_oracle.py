"""The numpy oracle of the compact read-back format against itself and against sizes worked out by hand (no GPU)."""
import numpy as np
import pytest

import compact_cases as cc


@pytest.mark.parametrize("case", cc.hand_cases(), ids=lambda c: c[0])
def test_hand_cases(case):
    name, t, nbytes, w, exc = case
    blob, st = cc.encode(np.zeros((0, 3), np.float32), t, 32)
    assert blob.nbytes == st["blobBytes"] == nbytes
    assert st["vertexBytes"] == 0 and st["triangleBytes"] == nbytes - 64 and st["groups"] == 1
    assert st["widthHistogram"][w] == 1 and sum(st["widthHistogram"]) == 1 and st["exceptions"] == exc
    offsets_at = cc.layout(blob)[2]
    assert blob[offsets_at] == 0 and blob[offsets_at + 1] == (nbytes - 64 - 8) // 4
    assert blob[offsets_at + 2] == t.min() and blob[offsets_at + 3] == (w | exc << 8)
    v, back = cc.decode(blob)
    assert len(v) == 0 and back.tobytes() == t.tobytes()


def test_header_and_padding():
    v = cc.ring_vertices(5, 2)
    t = np.array([[0, 1, 2], [2, 3, 4]], np.uint32)
    blob, st = cc.encode(v, t, 9)
    lo, hi = cc.extents(v)
    assert blob[:4].tolist() == [0x43534C4D, 1, 9, 64] and blob[:4].tobytes()[:4] == b"MLSC"
    assert blob[4:8].tolist() == [5, 0, 2, 0] and blob[14:16].tolist() == [len(blob), 0]
    assert blob[8:11].tobytes() == lo.tobytes() and blob[11:14].tobytes() == hi.tobytes()
    vwords = cc.layout(blob)[0]
    assert vwords == (15 * 9 + 31) // 32 == 5 and st["vertexBytes"] == 20
    assert blob[16 + vwords - 1] >> (15 * 9 - 32 * 4) == 0                       # the padding bits of the vertex stream
    # both ends of every axis are hit exactly: q = 0 and q = 2^b - 1 decode to lo and hi
    q = cc.unpack_bits(blob[16:16 + vwords], 15, 9).reshape(-1, 3)
    assert (q.min(axis=0) == 0).all() and (q.max(axis=0) == 511).all()
    got, _ = cc.decode(blob)
    assert (got.min(axis=0) == lo).all() and (got.max(axis=0) == hi).all()


def test_order_has_minus_zero_below_plus_zero():
    v = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0]], np.float32)
    lo, hi = cc.extents(v)
    assert np.signbit(lo[:2]).all() and not np.signbit(hi[:2]).any()
    blob, st = cc.encode(v, np.zeros((0, 3), np.uint32), 8)
    assert st["step"] == [0.0, 0.0, 0.0]                                        # d = 0 on every axis: q = 0
    assert not blob[16:18].any()
    got, _ = cc.decode(blob)
    assert (got == v).all()


@pytest.mark.parametrize("b", (8, 16, 21, 24, 32))
@pytest.mark.parametrize("V,T", ((0, 0), (1, 1), (63, 63), (64, 64), (65, 65), (1000, 257)))
def test_round_trip(b, V, T):
    v = cc.ring_vertices(V, V + b, offset=(1.0e6, -3.0, 0.0), scale=2.0)
    if V >= 8:
        v[:, 2] = 0.25                                                          # an axis with hi = lo
    t = cc.local_triangles(T, max(V, 1), seed=T)
    blob, st = cc.encode(v, t, b)
    assert blob.nbytes == st["blobBytes"] == 64 + st["vertexBytes"] + st["triangleBytes"]
    got_v, got_t = cc.decode(blob)
    assert got_t.tobytes() == t.tobytes()
    cc.check_vertices(got_v, v, b)


def test_arbitrary_indices_and_bits_come_back():
    rng = np.random.default_rng(5)
    t = rng.integers(0, 2 ** 32, (130, 3), dtype=np.uint64).astype(np.uint32)
    v = rng.integers(0, 2 ** 32, (7, 3), dtype=np.uint64).astype(np.uint32).view(np.float32)      # NaNs and infinities among them
    blob, st = cc.encode(v, t, 32)
    got_v, got_t = cc.decode(blob)
    assert got_t.tobytes() == t.tobytes() and got_v.tobytes() == v.tobytes()
    with pytest.raises(cc.Invalid):
        cc.encode(np.array([[0, np.nan, 0]], np.float32), t, 16)
    for b in (0, 7, 25, 31, 33):
        with pytest.raises(cc.Invalid):
            cc.encode(v, t, b)


def test_local_indices_take_a_third():
    """What the format is for: indices numbered as a sink numbers them."""
    t = cc.local_triangles(6400, 3300, spread=40, far=0.01, seed=1)
    blob, st = cc.encode(np.zeros((0, 3), np.float32), t, 32)
    assert st["triangleBytes"] < 0.36 * t.nbytes
    assert cc.decode(blob)[1].tobytes() == t.tobytes()
