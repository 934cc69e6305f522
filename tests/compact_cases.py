"""Numpy oracle of the compact read-back format (include/mlsgpu_hip.h, `mlsgpu_hip_mesh_compact`): `encode` makes the blob the
device has to make byte for byte, `decode` is the library decoder's counterpart, and the cases are shared by the CPU and GPU tests."""
import numpy as np

MAGIC = 0x43534C4D          # "MLSC" read as a little-endian word
VERSION = 1
GROUP = 64
HEADER_WORDS = 16
STAT_NAMES = ("numVertices", "numTriangles", "vertexBits", "blobBytes", "vertexBytes", "triangleBytes", "groups", "exceptions",
              "widthHistogram", "step")
STATS_BYTES = 8 * 8 + 33 * 8 + 3 * 8


class Invalid(ValueError):
    """MLSGPU_ERR_INVALID"""


class Format(ValueError):
    """MLSGPU_ERR_FORMAT"""


def valid_bits(b):
    return b == 32 or 8 <= b <= 24


def ordered(bits):
    """The order-preserving map from float bits to uint32 (-0 < +0), and back."""
    bits = np.asarray(bits, np.uint32)
    return np.where(bits >> 31, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def unordered(u):
    u = np.asarray(u, np.uint32)
    return np.where(u >> 31, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32)


def pack_bits(values, w):
    """values[i] occupies bits [i*w, (i+1)*w) of a stream whose bit j is bit j % 32 of word j // 32."""
    values = np.asarray(values, np.uint64)
    n = len(values)
    words = (n * w + 31) // 32
    out = np.zeros(words + 1, np.uint64)
    at = np.arange(n, dtype=np.uint64) * np.uint64(w)
    idx, sh = (at >> np.uint64(5)).astype(np.int64), at & np.uint64(31)
    wide = values << sh                                             # < 2^63: w <= 32, sh <= 31
    np.bitwise_or.at(out, idx, wide & np.uint64(0xFFFFFFFF))
    np.bitwise_or.at(out, idx + 1, wide >> np.uint64(32))
    assert out[words] == 0
    return out[:words].astype(np.uint32)


def unpack_bits(words, n, w):
    two = np.concatenate([np.asarray(words, np.uint32), np.zeros(1, np.uint32)]).astype(np.uint64)
    at = np.arange(n, dtype=np.uint64) * np.uint64(w)
    idx, sh = (at >> np.uint64(5)).astype(np.int64), at & np.uint64(31)
    wide = two[idx] | (two[idx + 1] << np.uint64(32))
    return ((wide >> sh) & np.uint64((1 << w) - 1)).astype(np.uint64)


def extents(vertices):
    """(lo, hi) float32 [3] by the integer order; zeros for no vertices.  Raises Invalid for a non-finite coordinate."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    bits = v.view(np.uint32)
    bad = int(np.count_nonzero((bits & np.uint32(0x7F800000)) == np.uint32(0x7F800000)))
    if bad:
        raise Invalid("%d vertex coordinates are not finite" % bad)
    if len(v) == 0:
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    u = ordered(bits)
    return unordered(u.min(axis=0)).view(np.float32), unordered(u.max(axis=0)).view(np.float32)


def steps(lo, hi, b):
    """(d, scale = (2^b - 1) / d, step = d / (2^b - 1)) in double per axis; scale = step = 0 where d = 0 and for b = 32."""
    d = hi.astype(np.float64) - lo.astype(np.float64)
    if b == 32:
        return d, np.zeros(3), np.zeros(3)
    top = np.float64(2 ** b - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(d == 0, 0.0, top / d)
        step = np.where(d == 0, 0.0, d / top)
    return d, scale, step


def quantise(vertices, lo, hi, b):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    d, scale, _ = steps(lo, hi, b)
    q = np.floor((v.astype(np.float64) - lo.astype(np.float64)) * scale + 0.5)
    q = np.clip(q, 0.0, float(2 ** b - 1))
    return np.where(d == 0, 0.0, q).astype(np.uint64)


def plan_group(idx):
    """(base, w, exceptions) of one group's 3n indices in slot order."""
    idx = np.asarray(idx, np.uint64)
    base = int(idx.min())
    v = idx - np.uint64(base)
    length = np.array([int(x + 1).bit_length() for x in v.tolist()])    # v >= 2^w - 1  <=>  bit_length(v + 1) > w
    best = None
    for w in range(1, 33):
        exc = int(np.count_nonzero(length > w)) if w < 32 else 0
        cost = 4 * ((len(idx) * w + 31) // 32) + 4 * exc
        if best is None or cost < best[0]:
            best = (cost, w, exc)
    return base, best[1], best[2]


def encode_group(idx):
    idx = np.asarray(idx, np.uint64)
    base, w, exc = plan_group(idx)
    v = idx - np.uint64(base)
    if w < 32:
        escape = np.uint64(2 ** w - 1)
        out = v >= escape
        slots = np.where(out, escape, v)
        tail = v[out].astype(np.uint32)
    else:
        slots, tail = v, np.zeros(0, np.uint32)
    assert len(tail) == exc
    return np.concatenate([np.array([base, w | exc << 8], np.uint32), pack_bits(slots, w), tail]), w, exc


def encode(vertices, triangles, b):
    """The blob as a uint32 array, and the statistics as a dict."""
    if not valid_bits(b):
        raise Invalid("vertexBits %d" % b)
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.uint32).reshape(-1, 3)
    V, T = len(v), len(t)
    if b == 32:
        lo = hi = np.zeros(3, np.float32)
        vsec = v.view(np.uint32).reshape(-1).copy()
    else:
        lo, hi = extents(v)
        vsec = pack_bits(quantise(v, lo, hi, b).reshape(-1), b)
    G = (T + GROUP - 1) // GROUP
    records, offsets, hist, exceptions = [], [0], [0] * 33, 0
    flat = t.reshape(-1)
    for g in range(G):
        rec, w, exc = encode_group(flat[3 * GROUP * g:3 * GROUP * (g + 1)])
        records.append(rec)
        offsets.append(offsets[-1] + len(rec))
        hist[w] += 1
        exceptions += exc
    if offsets[-1] >= 2 ** 32:
        raise OverflowError
    tsec = np.concatenate([np.array(offsets, np.uint32)] + records)
    total = HEADER_WORDS + len(vsec) + len(tsec)
    head = np.zeros(HEADER_WORDS, np.uint32)
    head[0:4] = (MAGIC, VERSION, b, GROUP)
    head[4:6] = (V & 0xFFFFFFFF, V >> 32)
    head[6:8] = (T & 0xFFFFFFFF, T >> 32)
    head[8:11] = lo.view(np.uint32)
    head[11:14] = hi.view(np.uint32)
    head[14:16] = (total & 0xFFFFFFFF, total >> 32)
    stats = {"numVertices": V, "numTriangles": T, "vertexBits": b, "blobBytes": 4 * total, "vertexBytes": 4 * len(vsec),
             "triangleBytes": 4 * len(tsec), "groups": G, "exceptions": exceptions, "widthHistogram": hist,
             "step": [float(x) for x in steps(lo, hi, b)[2]]}
    return np.concatenate([head, vsec, tsec]), stats


def decode(blob):
    """(vertices float32 [V, 3], triangles uint32 [T, 3]) of a blob (uint32 array or bytes).  Raises Format."""
    raw = blob.tobytes() if isinstance(blob, np.ndarray) else bytes(blob)
    if len(raw) % 4 or len(raw) < 4 * HEADER_WORDS:
        raise Format("length")
    words = np.frombuffer(raw, np.uint32)
    if words[0] != MAGIC or words[1] != VERSION or not valid_bits(int(words[2])) or words[3] != GROUP:
        raise Format("header")
    b = int(words[2])
    V, T, total = (int(words[k]) | int(words[k + 1]) << 32 for k in (4, 6, 14))
    if V >= 2 ** 32 or 3 * T >= 2 ** 32 or total != len(words):
        raise Format("sizes")
    lo, hi = words[8:11].view(np.float32), words[11:14].view(np.float32)
    if b == 32:
        if words[8:14].any():
            raise Format("extent")
    elif not (np.isfinite(lo).all() and np.isfinite(hi).all() and (ordered(words[8:11]) <= ordered(words[11:14])).all()):
        raise Format("extent")
    vwords = 3 * V if b == 32 else (3 * V * b + 31) // 32
    G = (T + GROUP - 1) // GROUP
    if HEADER_WORDS + vwords + G + 1 > total:
        raise Format("sections")
    vsec = words[HEADER_WORDS:HEADER_WORDS + vwords]
    if b == 32:
        vertices = vsec.view(np.float32).reshape(-1, 3).copy()
    else:
        q = unpack_bits(vsec, 3 * V, b).reshape(-1, 3)
        vertices = (lo.astype(np.float64) + q.astype(np.float64) * steps(lo, hi, b)[2]).astype(np.float32)
    offsets = words[HEADER_WORDS + vwords:][:G + 1].astype(np.int64)
    records = words[HEADER_WORDS + vwords + G + 1:]
    if offsets[0] != 0 or offsets[-1] != len(records) or (np.diff(offsets) < 2).any():
        raise Format("offsets")
    out = np.zeros(3 * T, np.uint32)
    for g in range(G):
        rec = records[offsets[g]:offsets[g + 1]]
        n = min(GROUP, T - GROUP * g)
        base, w, exc = int(rec[0]), int(rec[1]) & 0xFF, int(rec[1]) >> 8
        if not 1 <= w <= 32 or exc > 3 * n:
            raise Format("record")
        pw = (3 * n * w + 31) // 32
        if len(rec) != 2 + pw + exc:
            raise Format("record length")
        val = unpack_bits(rec[2:2 + pw], 3 * n, w)
        if w < 32:
            esc = val == np.uint64(2 ** w - 1)
            if int(np.count_nonzero(esc)) != exc:
                raise Format("escapes")
            val[esc] = rec[2 + pw:].astype(np.uint64)
        elif exc:
            raise Format("escapes")
        val += np.uint64(base)
        if (val >= np.uint64(2 ** 32)).any():
            raise Format("wrap")
        out[3 * GROUP * g:3 * GROUP * g + 3 * n] = val.astype(np.uint32)
    return vertices, out.reshape(-1, 3)


def layout(blob):
    """Where the sections of a well-formed blob (uint32 array) begin, in words: (vertex words, G, offsets at, records at)."""
    b, V, T = int(blob[2]), int(blob[4]), int(blob[6])
    vwords = 3 * V if b == 32 else (3 * V * b + 31) // 32
    G = (T + GROUP - 1) // GROUP
    return vwords, G, HEADER_WORDS + vwords, HEADER_WORDS + vwords + G + 1


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)).astype(np.float64) - x.astype(np.float64))


def vertex_bound(lo, hi, b):
    """The contract's bound on |x' - x| per axis: 0.5 d / (2^b - 1) + ulp32(max(|lo|, |hi|))."""
    d = hi.astype(np.float64) - lo.astype(np.float64)
    return 0.5 * d / float(2 ** b - 1) + ulp32(np.maximum(np.abs(lo), np.abs(hi)))


def check_vertices(got, vertices, b):
    """Exact at b = 32 (as bits), within the bound below."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    assert got.shape == v.shape and got.dtype == np.float32
    if b == 32:
        assert got.tobytes() == v.tobytes()
    elif len(v):
        lo, hi = extents(v)
        err = np.abs(got.astype(np.float64) - v.astype(np.float64))
        assert (err <= vertex_bound(lo, hi, b)).all(), (b, err.max(axis=0), vertex_bound(lo, hi, b))


def same_stats(got, want):
    assert list(got) == list(STAT_NAMES)
    for name in STAT_NAMES:
        assert got[name] == want[name], (name, got[name], want[name])


# ---------------------------------------------------------------- cases

def ring_vertices(n, seed=0, offset=(0.0, 0.0, 0.0), scale=1.0):
    """n vertices with negative coordinates, both zeros and, with an offset, coordinates near 10^6."""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1.0, 1.0, (n, 3)) * scale + np.asarray(offset)).astype(np.float32)
    if n >= 4:
        v[1, 0], v[2, 0] = 0.0, -0.0
    return v


def local_triangles(T, V, spread=40, far=0.02, seed=0):
    """T triangles whose indices lie near 3t * V / (3T), as a sink numbers them, with a few corners welded far away."""
    rng = np.random.default_rng(seed)
    if V == 0:
        return np.zeros((0, 3), np.uint32)
    centre = (np.arange(T, dtype=np.int64) * max(V - 1, 1)) // max(T, 1)
    t = centre[:, None] + rng.integers(-spread, spread + 1, (T, 3))
    away = rng.random((T, 3)) < far
    t = np.where(away, rng.integers(0, V, (T, 3)), t)
    return np.clip(t, 0, V - 1).astype(np.uint32)


def hand_cases():
    """(name, triangles, blob bytes at b = 32 with no vertices, w of the first group, its exceptions), sizes worked out by hand:
    64 header bytes + 4 (G + 1) offset bytes + per group 8 + 4 ceil(3 n w / 32) + 4 exceptions."""
    cases = []
    # all indices equal: every v is 0 < 2^1 - 1, so w = 1 holds them in ceil(192 / 32) = 6 words and nothing is cheaper
    cases.append(("equal", np.full((64, 3), 7, np.uint32), 64 + 8 + 8 + 24, 1, 0))
    # one triangle, v = (0, 0, 14), 14 = 2^4 - 2: inline at w = 4 (one word); w < 4 costs one word and one exception
    cases.append(("inline_2w_minus_2", np.array([[5, 5, 19]], np.uint32), 64 + 8 + 8 + 4, 4, 0))
    # a full group of v in {0, 1, 2} and one v = 3: at w = 2 the 2 = 2^2 - 2 is inline and the 3 = 2^2 - 1 an exception (12 words
    # + 1); w = 3 holds the 3 inline for 18 words, w = 1 escapes every v >= 1
    t = (np.arange(192, dtype=np.uint32) % 3).reshape(64, 3) + 100
    t[10, 1] = 103
    cases.append(("exception_2w_minus_1", t, 64 + 8 + 8 + 4 * 12 + 4, 2, 1))
    # a tie: 11 triangles (33 slots), v = 0 except one v = 1.  w = 1: ceil(33 / 32) = 2 words + 1 exception; w = 2: ceil(66 / 32)
    # = 3 words: 12 bytes each, and the smaller w wins
    t = np.zeros((11, 3), np.uint32) + 9
    t[4, 2] = 10
    cases.append(("tie_takes_smaller_w", t, 64 + 8 + 8 + 4 * 2 + 4, 1, 1))
    # a full group with base 0 and 191 values from 2^32 - 2 down: any w < 32 escapes all 191 (6 w words + 191 >= 197 words),
    # w = 32 holds them in 192 words
    F = 2 ** 32 - 2
    t = (F - np.arange(192, dtype=np.uint64)).astype(np.uint32).reshape(64, 3)
    t[63, 2] = 0
    cases.append(("spans_0_to_2_32_minus_2", t, 64 + 8 + 8 + 4 * 192, 32, 0))
    return cases
