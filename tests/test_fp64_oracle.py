"""The oracle against a float64 restatement of the mathematics (tests/fp64_reference.py), not against itself.

Every other kernel test asks whether the HIP output is bit-identical to the oracle.  These ask whether the oracle's MLS field
and marching mesh are what the method defines, within a tolerance measured from float32 rounding, at the octree settings,
shapes, boundary limits and special field values where a restatement could quietly go wrong; and prove, with known-wrong
inputs, that the comparisons would notice.  test_gpu_fp64.py holds the kernels to the same references."""
import numpy as np
import pytest

import fp64_reference as fr
import oracle_binding as ob
from mlsgpu_amd import synth
from test_oracle_marching import GENERATE_CASES, host_generator

TREES = [(6, 3), (4, 4), (3, 5), (7, 3)]            # (levels, subsampling)
LIMITS = [0.0, 0.5, 1.0, 1.5, 3.0]
MAX_AMBIGUOUS = 0.01


# ---- clouds: (splats, grid size (none a multiple of 8), offset) ------------------------------------------------------------

def planes_cloud(n, seed):
    """Two parallel planes 4.3 cells apart, normals facing away from each other (a thin slab)."""
    rng = np.random.default_rng(seed)
    s = np.zeros(n, ob.SPLAT_DTYPE)
    top = rng.random(n) < 0.5
    s["position"][:, 0] = rng.uniform(2, 30, n)
    s["position"][:, 1] = rng.uniform(2, 30, n)
    s["position"][:, 2] = np.where(top, 17.6, 13.3)
    s["normal"][:, 2] = np.where(top, 1.0, -1.0)
    s["radius"] = rng.uniform(1.5, 3.0, n)
    s["quality"] = rng.uniform(0.2, 1.0, n)
    return s


def make_mls_cloud(name):
    if name == "sphere":
        return synth.sphere_cloud(6000, (20.5, 19.25, 21.0), 14.0, 1.0, 2.5, 11), (43, 41, 45), (0, 0, 0)
    if name == "uniform":       # radii 0.5 - 9: splats on several octree levels
        return synth.uniform_cloud(1500, 40.0, 0.5, 9.0, 12), (41, 41, 41), (0, 0, 0)
    if name == "shells":
        return synth.shells_cloud(8000, 47.0, 6.0, 1.0, 2.0, 13), (47, 46, 45), (0, 0, 0)
    if name == "planes":
        return planes_cloud(3000, 14), (33, 34, 31), (0, 0, 0)
    if name == "negative_offset":
        off = (-37, -21, -50)
        s = synth.sphere_cloud(5000, (16.0, 15.5, 17.25), 11.0, 1.0, 2.0, 15)
        s["position"] += np.array(off, np.float32)
        return s, (35, 33, 37), off
    raise KeyError(name)


MLS_CLOUDS = ["sphere", "uniform", "shells", "planes", "negative_offset"]


def sample_corners(splats, size, offset, seed=1, n=3000, blocks=2, uniform=500):
    """Seeded local corner coordinates [k, 3]: n near random splats, every corner of `blocks` whole 8^3 blocks that hold a
    splat, and `uniform` anywhere in the grid."""
    rng = np.random.default_rng(seed)
    size, offset = np.array(size), np.array(offset)
    idx = rng.integers(0, len(splats), n)
    near = np.rint(splats["position"][idx].astype(np.float64) + rng.uniform(-2.5, 2.5, (n, 3))).astype(np.int64) - offset
    parts = [np.clip(near, 0, size - 1), rng.integers(0, size, (uniform, 3))]
    cube = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for b in range(blocks):
        base = (np.floor(splats["position"][idx[b]] - offset).astype(np.int64) // 8) * 8
        parts.append(np.clip(base + cube, 0, size - 1))
    return np.unique(np.concatenate(parts), axis=0)


def oracle_field(splats, commands, start, size, offset, subsampling, shape, limit):
    """The oracle's processCorners over the whole grid, one swathe: field[z * H8 + y, x]."""
    W8, H8, D8 = [(x + 7) // 8 * 8 for x in size]
    field = np.full((H8 * D8, W8), -7.0, np.float32)
    ob.process_corners(field, splats, commands, start, subsampling, offset, size[0], size[1], H8, 0, 0, size[2] - 1,
                       ob.lib().orc_boundary_factor(limit), shape)
    return field, H8


def at(field, h8, corners):
    return field[corners[:, 2] * h8 + corners[:, 1], corners[:, 0]]


_SUMS = {}


def cloud_and_sums(name):
    """(raw cloud, size, offset, sampled corners, fp64 sums): the fp64 sums depend on the cloud and corners only."""
    if name not in _SUMS:
        cloud, size, offset = make_mls_cloud(name)
        mutated = cloud.copy()
        ob.Tree(mutated, 0, len(mutated), size, offset, 3, 6)           # radius -> 1/r^2, as every kernel reads it
        corners = sample_corners(cloud, size, offset)
        _SUMS[name] = (cloud, size, offset, corners, fr.mls_sums_fp64(mutated, corners + np.array(offset)))
    return _SUMS[name]


def check_field(got, s, shape, limit, what, min_values=200):
    bf = np.float64(ob.lib().orc_boundary_factor(limit))
    exp, amb = fr.mls_finish_fp64(s, shape, bf)
    c = fr.compare_field(got, exp, amb)
    e = c["err"]
    assert c["ambiguous"] < MAX_AMBIGUOUS, (what, c["ambiguous"])
    assert c["nan_mismatch"] == 0, (what, c["nan_mismatch"])
    if limit > 0:
        assert c["values"] >= min_values, what      # the comparison is not over NaNs only
    if len(e):
        assert e.max() <= fr.MLS_MAX_ABS, (what, e.max())
        assert np.percentile(e, 99) <= fr.MLS_P99_ABS, (what, np.percentile(e, 99))
    return c


def test_boundary_factor_fp64():
    for limit in LIMITS:
        assert abs(ob.lib().orc_boundary_factor(limit) - fr.boundary_factor_fp64(limit)) <= 1e-6 * max(1, limit * limit)


@pytest.mark.parametrize("name", MLS_CLOUDS)
def test_oracle_mls_field_vs_fp64(name):
    """The oracle's field at every tree setting, both shapes and five boundary limits against the brute-force fp64 field:
    NaN exactly where fp64 has NaN, values within the pinned tolerances, on all but a small ambiguous share."""
    cloud, size, offset, corners, s = cloud_and_sums(name)
    for levels, sub in TREES:
        mutated = cloud.copy()
        t = ob.Tree(mutated, 0, len(mutated), size, offset, sub, levels)
        for shape in (0, 1):
            for limit in LIMITS:
                field, h8 = oracle_field(mutated, t.commands, t.start, size, offset, sub, shape, limit)
                check_field(at(field, h8, corners), s, shape, limit, (name, levels, sub, shape, limit))


# ---- sensitivity: the MLS comparison fails on known-wrong inputs ---------------------------------------------------------

def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _sphere_setup():
    cloud, size, offset, corners, s = cloud_and_sums("sphere")
    mutated = cloud.copy()
    t = ob.Tree(mutated, 0, len(mutated), size, offset, 3, 6)
    return cloud, mutated, t, size, offset, corners, s


def test_sensitivity_baseline_passes():
    """The unaltered inputs of the sensitivity tests below pass the comparison (so what fails there is the alteration)."""
    cloud, mutated, t, size, offset, corners, s = _sphere_setup()
    field, h8 = oracle_field(mutated, t.commands, t.start, size, offset, 3, 0, 1.0)
    check_field(at(field, h8, corners), s, 0, 1.0, "baseline")


def test_sensitivity_dropped_splat():
    """One splat that hits corners of a block is taken out of that block's list: the comparison fails."""
    cloud, mutated, t, size, offset, corners, s = _sphere_setup()
    block = (np.floor(cloud["position"][0]).astype(np.int64) // 8) * 8
    cube = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
    bc = np.clip(block + cube, 0, np.array(size) - 1)
    bs = fr.mls_sums_fp64(mutated, bc.astype(np.float64))
    # the heaviest splat of the block: largest summed weight over its corners
    x = mutated["position"][None, :, :].astype(np.float64) - bc[:, None, :]
    d = (x * x).sum(-1) * mutated["radius"][None, :]
    w = np.where(d < 0.99, (1 - d) ** 4 * mutated["quality"][None, :], 0).sum(0)
    victim = int(np.argmax(w))
    code = ob.lib().orc_make_code(*[int(v) for v in block]) >> 9
    cmds = t.commands.copy()
    pos = int(t.start[code])
    found = False
    while pos >= 0 and not found:          # walk the list; swap the victim to the end of its range, then end the range there
        end = int(cmds[pos])
        ids = cmds[pos + 1:end]
        hit = np.nonzero(ids == victim)[0]
        if len(hit):
            ids[hit[0]], ids[-1] = ids[-1], -1
            found = True
        pos = int(cmds[end])
    assert found
    field, h8 = oracle_field(mutated, cmds, t.start, size, offset, 3, 0, 1.0)
    assert _fails(lambda: check_field(at(field, h8, bc), bs, 0, 1.0, "dropped", 20))
    field, h8 = oracle_field(mutated, t.commands, t.start, size, offset, 3, 0, 1.0)
    check_field(at(field, h8, bc), bs, 0, 1.0, "intact", 20)


def test_sensitivity_offset_by_one_cell():
    cloud, mutated, t, size, offset, corners, s = _sphere_setup()
    shifted = (offset[0] + 1, offset[1], offset[2])
    t2 = ob.Tree(cloud.copy(), 0, len(cloud), size, shifted, 3, 6)
    field, h8 = oracle_field(mutated, t2.commands, t2.start, size, shifted, 3, 0, 1.0)
    assert _fails(lambda: check_field(at(field, h8, corners), s, 0, 1.0, "offset"))


def test_sensitivity_weight_power():
    """fp64 with the weight (1 - d)^2 instead of (1 - d)^4 disagrees with the oracle."""
    cloud, mutated, t, size, offset, corners, s = _sphere_setup()
    s2 = fr.mls_sums_fp64(mutated, corners + np.array(offset), weight_power=2)
    field, h8 = oracle_field(mutated, t.commands, t.start, size, offset, 3, 0, 1.0)
    assert _fails(lambda: check_field(at(field, h8, corners), s2, 0, 1.0, "weight"))
    field, h8 = oracle_field(mutated, t.commands, t.start, size, offset, 3, 1, 1.0)
    assert _fails(lambda: check_field(at(field, h8, corners), s2, 1, 1.0, "weight plane"))


# ---- marching -------------------------------------------------------------------------------------------------------------

F32 = np.finfo(np.float32)
DENORM = np.float32(1e-45)                      # the smallest positive denormal
BELOW_MAX = np.nextafter(F32.max, np.float32(0))
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
SPECIAL_PALETTES = {
    "zeros": [0.0, -0.0, 1.0, -1.0],
    "denormals": [0.0, -0.0, DENORM, -DENORM, 1.0, -1.0, F32.tiny, -F32.tiny],
    "flt_max": [F32.max, -F32.max, BELOW_MAX, -BELOW_MAX, 1.0, -1.0, 0.0, -0.0],
    "nonfinite": [np.inf, -np.inf, np.nan, NEG_NAN, 1.0, -1.0, 0.5, -0.0],
    "mixed": [0.0, -0.0, 1.0, -1.0, DENORM, -DENORM, F32.max, -F32.max, BELOW_MAX, np.inf, -np.inf, np.nan, NEG_NAN, 0.25],
}


def special_field(name, size=(13, 12, 11), seed=3):
    """A seeded 3-D pattern [z, y, x] over the palette, with a +-1 checkerboard on every fourth z slice so that ordinary
    values sit next to the special ones."""
    pal = np.array(SPECIAL_PALETTES[name], np.float32)
    rng = np.random.default_rng(seed + len(name))
    W, H, D = size
    f = pal[rng.integers(0, len(pal), (D, H, W))]
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    chk = np.where((x + y + z) % 2 == 0, np.float32(1.0), np.float32(-1.0))
    return np.where(z % 4 == 2, chk, f).astype(np.float32)


def field_of(fn, size):
    W, H, D = size
    ys, xs = np.meshgrid(np.arange(H, dtype=np.uint32), np.arange(W, dtype=np.uint32), indexing="ij")
    return np.stack([np.asarray(fn(xs, ys, z), np.float32) for z in range(D)])


def torus_field(size=(41, 39, 31), c=(20.3, 19.1, 15.6), big=11.2, small=4.3):
    W, H, D = size
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    r = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2)
    return (np.sqrt((r - big) ** 2 + (z - c[2]) ** 2) - small).astype(np.float32)


MARCH_CASES = sorted(GENERATE_CASES) + ["torus"] + ["special_" + k for k in sorted(SPECIAL_PALETTES)]
# closed surfaces: Euler characteristic (the field is negative inside, so a positive signed volume)
CLOSED = {"sphere": 2, "torus": 0}


def march_field(name):
    if name in GENERATE_CASES:
        _, size, fn = GENERATE_CASES[name]
        return field_of(fn, size)
    if name == "torus":
        return torus_field()
    return special_field(name[len("special_"):])


def oracle_march(field, mem_slices=1000, swathe=8):
    D, H, W = field.shape
    mw, mh, md = W + 3, H + 2, max(D, 8) + 5        # (maxDepth below the z alignment would leave no swathe at all)
    m = ob.MarchingOracle(mw, mh, md, swathe, (mw - 1) * (mh - 1) * 872 * mem_slices, (8, 8, 8))
    return m.generate(host_generator(lambda x, y, z: field[z]), (W, H, D)), m.stats()


def check_mesh(batches, ref, name):
    c = fr.compare_mesh(batches, ref)
    assert c["missing"] == 0 and c["extra"] == 0, (name, c["missing"], c["extra"])
    assert c["triangles_match"], (name, c["triangles"], ref["triangles"])
    assert c["off_tetrahedron"] == 0, name
    assert c["max_err"] <= fr.MARCH_TOL, (name, c["max_err"])
    # every vertex, flagged edges included, is what IEEE float32 gives for iso0 * (1 / (iso0 - iso1)) with denormals
    # kept: the oracle's behaviour on the special values, pinned (the GPU tests hold the kernels to it bit for bit)
    assert c["f32_pinned"], name
    if name in CLOSED:
        assert c["euler"] == CLOSED[name], (name, c["euler"])
        assert c["volume"] > 0, name
    return c


@pytest.mark.parametrize("name", MARCH_CASES)
def test_oracle_marching_vs_fp64(name):
    field = march_field(name)
    ref = fr.marching_fp64(field)
    batches, st = oracle_march(field)
    assert len(ref["edges"]) > 0 and ref["triangles"] > 0
    c = check_mesh(batches, ref, name)
    assert st["welded"] == c["vertices"] and st["indices"] == 3 * c["triangles"]
    if name in ("special_denormals", "special_flt_max", "special_mixed"):
        assert ref["flagged"].any(), name          # the field does reach the edges float32 cannot follow
    if name in ("special_zeros", "special_nonfinite"):
        assert not ref["flagged"].any()
    # two slices of mesh memory: several ship-outs, the same welded mesh
    small, _ = oracle_march(field, mem_slices=2)
    check_mesh(small, ref, name)


# What the oracle does on one edge from iso0 (at p) to iso1 (at p + d): the vertex p + t d with t as below, in float32 with
# denormals kept.  fp64 says t = iso0 / (iso0 - iso1); "flagged" marks where float32 cannot follow it.
EDGE_CASES = [
    # iso0, iso1, t the oracle produces, flagged
    (np.float32(0.0), np.float32(-1.0), np.float32(0.0), False),           # +0 is outside: vertex at p
    (np.float32(-0.0), np.float32(-1.0), np.float32(-0.0), False),         # -0 is outside too (iso >= 0), t = -0: at p
    (np.float32(-0.0), np.float32(0.0), None, None),                       # both outside: no vertex
    (np.float32(-1.0), np.float32(-0.0), np.float32(1.0), False),          # inside -> -0 (outside): at p + d
    (DENORM, np.float32(-1.0), DENORM, False),                             # denormal kept: t = 1e-45
    (np.float32(0.0), -DENORM, np.float32(np.nan), True),                  # 1 / 1e-45 = inf, 0 * inf: NaN vertex
    (DENORM, -DENORM, np.float32(np.inf), True),                           # 1 / 2.8e-45 = inf: t = inf (fp64: 0.5)
    (F32.max, -F32.max, np.float32(0.0), True),                            # difference inf, 1/inf = 0: at p (fp64: 0.5)
    (F32.max, np.float32(-1.0), np.float32(1.0) - np.float32(2.0 ** -24), True),   # 1/FLT_MAX = 2^-128 is denormal: t =
    #                                                                        FLT_MAX * 2^-128 = 1 - 2^-24 (flushed: t = 0)
    (np.float32(1.0), -F32.max, np.float32(1.0 / float(F32.max)), True),  # t denormal (2.9e-39), vertex at p
]


@pytest.mark.parametrize("iso0,iso1,t,flagged", EDGE_CASES)
def test_oracle_special_edge(iso0, iso1, t, flagged):
    """One cell whose corner 0 holds iso0 and the other seven iso1: seven edges from corner 0, each vertex at t d."""
    field = np.full((2, 2, 2), iso1, np.float32)
    field[0, 0, 0] = iso0
    ref = fr.marching_fp64(field)
    if t is None:
        assert len(ref["edges"]) == 0 and ref["triangles"] == 0
        assert oracle_march(field)[0] == []
        return
    assert len(ref["edges"]) == 7 and np.all(ref["flagged"] == flagged)
    batches, _ = oracle_march(field)
    v, _ = fr.weld(batches)
    with np.errstate(invalid="ignore"):       # p + t d with p = 0: -0 becomes +0, and inf * 0 is NaN off the edge's axes
        exp = np.float32(0.0) + fr.DIRECTIONS.astype(np.float32) * t
    assert fr.same_vertex_multiset(v, exp), (v, exp)
    assert fr.same_vertex_multiset(v, ref["pos_f32"])


# ---- sensitivity: the marching comparison fails on known-wrong inputs ----------------------------------------------------

def test_sensitivity_zero_convention():
    """A reference that calls 0.0 inside (a sign-bit test gets -0.0 so) does not match the oracle's mesh."""
    field = special_field("zeros")
    batches, _ = oracle_march(field)
    check_mesh(batches, fr.marching_fp64(field), "zeros")
    wrong = np.where(field == 0, np.float32(-F32.tiny), field).astype(np.float32)
    c = fr.compare_mesh(batches, fr.marching_fp64(wrong))
    assert not fr.mesh_ok(c)
    neg = np.where((field == 0) & np.signbit(field), np.float32(-F32.tiny), field).astype(np.float32)   # -0.0 only
    assert not fr.mesh_ok(fr.compare_mesh(batches, fr.marching_fp64(neg)))


def test_sensitivity_moved_vertex():
    field = torus_field()
    ref = fr.marching_fp64(field)
    batches, _ = oracle_march(field)
    assert fr.mesh_ok(fr.compare_mesh(batches, ref))
    moved = [dict(b) for b in batches]
    moved[0]["vertices"] = moved[0]["vertices"].copy()
    moved[0]["vertices"][0, 0] += np.float32(0.01)
    c = fr.compare_mesh(moved, ref)
    assert c["missing"] == 1 and c["extra"] == 1 and not fr.mesh_ok(c)
