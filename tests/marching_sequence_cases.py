"""Sequences of unlike buckets on ONE marching object (test_marching_sequences_oracle.py on the CPU,
test_gpu_marching_sequences.py on the device), and generators that fill the field image's padding with something other than
zeros.

A worker's marching object is created at the worker's maximum and lives as long as the worker; beginGenerate sets layout,
wideKeys, direct, offsets, zTop and the swathe's zBias per call, while the field image (pitch and slice stride from the
MAXIMUM dims), the lattice words and rows, the cell codes, the key scratch of either width and the slice histogram keep what
the bucket before left there.  An Obj here is such an object (dims, swathe, mesh memory), a Step one bucket marched on it; what
a step must give is the oracle's run of that bucket on a FRESH object of the same dims, swathe and memory (oracle_step), so a
result may not depend on what the object marched before.

Every step states the weld it takes (lattice: the bucket fits one swathe; sort: it does not, or MLSGPU_HIP_WELD=sort), the
triangle route of a lattice step (rows or cells; the sort weld emits per cell and has none), its swathes and whether it
overflows at each memory setting; test_marching_sequences_oracle.py asserts all of them."""
import functools
import time

import numpy as np

import marching_extent_cases as mx
import marching_key_cases as mk
import oracle_binding as ob

OFFSETS = (mx.KEY_OFFSET, (100, 9, 0))       # key offsets of the steps at even and odd places of a sequence


class Obj:
    """A marching object: `dims` maximum corners, `swathe` maximum slices a swathe, mesh memory by name (mx.Case.memory)."""

    def __init__(self, name, dims, swathe):
        self.name, self.dims, self.swathe = name, tuple(dims), swathe
        self.max_swathe = min(swathe, dims[2]) // mx.ALIGNMENT[2] * mx.ALIGNMENT[2]
        self.sort_buffers = self.max_swathe < dims[2]
        self.pitch = -(-dims[0] // mx.ALIGNMENT[0]) * mx.ALIGNMENT[0]
        self.z_stride = -(-dims[1] // mx.ALIGNMENT[1]) * mx.ALIGNMENT[1]
        # rows of the field image (mlsgpu_marching::fieldRows): what a generator may write at all
        self.field_rows = self.z_stride * (self.max_swathe + 1 + mx.ALIGNMENT[2])

    def __repr__(self):
        return self.name

    def memory(self, which):
        slices = {"ample": self.dims[2], "tight": 2, "floor": 1}[which]
        return (self.dims[0] - 1) * (self.dims[1] - 1) * mx.MAX_CELL_BYTES * slices


class Step:
    """One bucket of a sequence.  `route`: "rows", "cells" or None (no lattice ship-out: sort weld, or no surface); `weld`:
    "lattice" or "sort"; `swathes`: how many the object cuts it into; `overflows`: the memory settings at which it does;
    `force_sort`: MLSGPU_HIP_WELD=sort is set for this step alone."""

    def __init__(self, name, field, size, route, weld, swathes=1, overflows=(), key_offset=mx.KEY_OFFSET, fn=None,
                 force_sort=False):
        self.name, self.field, self.size = name, field, tuple(size)
        self.route, self.weld, self.swathes, self.overflows = route, weld, swathes, tuple(overflows)
        self.key_offset, self.fn, self.force_sort = tuple(key_offset), fn or mx.FIELDS[field], force_sort

    def __repr__(self):
        return self.name

    @property
    def cells(self):
        return (self.size[0] - 1) * (self.size[1] - 1) * (self.size[2] - 1)

    @property
    def surface(self):
        return self.field != "positive"


def oracle_step(obj, step, memory):
    """(batches, stats) of a FRESH oracle object of the sequence object's dims, swathe and memory on one step; through the
    cache of marching_extent_cases, so a bucket that several sequences (or the key tests) march is computed once."""
    return mx._oracle_run(step.fn, step.size, obj.dims, obj.swathe, obj.memory(memory), step.key_offset)


def oracle_step_seconds(obj, step, memory):
    oracle_step(obj, step, memory)
    return mx.ORACLE_SECONDS[step.fn, step.size, obj.dims, obj.swathe, obj.memory(memory), step.key_offset]


def _numbered(steps):
    """Key offsets by place, OFFSETS[0] at even and OFFSETS[1] at odd ones, so that no two neighbours share theirs"""
    for i, s in enumerate(steps):
        s.key_offset = OFFSETS[i % 2]
    return steps


# ---- wide: one swathe always, no sort buffers ------------------------------------------------------------------------------
# Tight memory is two slices of the OBJECT's cells, 2051 x 19 x 2 x 13 = 1.01 M vertices: a step overflows there when its
# own mesh is larger, which the short rows' are not (56 k vertices on 32 x 17 x 13) and the tube's never is.
WIDE = Obj("wide", (2052, 20, 24), 24)
WIDE_STEPS = _numbered([
    Step("w_full", "noise", (2052, 20, 24), "cells", "lattice", overflows=("tight",)),      # size == dims; nw 65
    Step("w_nw1", "noise", (32, 17, 13), "rows", "lattice"),
    Step("w_tube2049", "tube", (2049, 17, 13), "cells", "lattice"),
    Step("w_nw2", "noise", (33, 5, 4), "rows", "lattice"),
    Step("w_nw33", "noise", (1025, 20, 13), "rows", "lattice", overflows=("tight",)),
    Step("w_nw64", "noise", (2048, 17, 13), "rows", "lattice", overflows=("tight",)),       # the widest rows-route launch
    Step("w_positive", "positive", (449, 17, 13), None, "lattice"),
    Step("w_nw1_again", "noise", (32, 17, 13), "rows", "lattice"),                        # equals w_nw1 byte for byte
])
assert WIDE_STEPS[1].key_offset == WIDE_STEPS[7].key_offset

# ---- deep: maxSwathe 64 < maxDepth 264, sort buffers ---------------------------------------------------------------------
DEEP = Obj("deep", (67, 35, 264), 64)
DEEP_STEPS = _numbered([
    Step("d_257", "noise", (65, 33, 257), None, "sort", swathes=5, overflows=("tight",)),
    Step("d_64", "noise", (65, 33, 64), "rows", "lattice", overflows=("tight",)),            # exactly one swathe
    Step("d_65", "noise", (17, 9, 65), None, "sort", swathes=2, overflows=("tight",)),       # the second swathe of one slice
    Step("d_2", "noise", (65, 33, 2), "rows", "lattice"),
    Step("d_full_tube", "tube", (67, 35, 264), None, "sort", swathes=5),                     # size == dims
    Step("d_tube40", "tube", (33, 33, 40), "cells", "lattice"),
    Step("d_64_forced", "noise", (65, 33, 64), None, "sort", overflows=("tight",), force_sort=True),
])

# ---- keys: the object of marching_key_cases' k34 ------------------------------------------------------------------------------
# k34 is 257 x 513 x 1033 (34-bit keys, 17 swathes of 64); its object is 260 x 515 x 1040, swathe 64, memory at the floor.
K34 = mk.case("k34", "swathes")
KEYS = Obj("keys", K34.dims, K34.swathe)
assert KEYS.memory(mk.MEMORY) == K34.memory(mk.MEMORY) and KEYS.max_swathe == K34.max_swathe == 64
# k32_b (512 x 513 x 257) clipped to the object: 260 x 513 x 257 has (10, 11, 10) bits and the flag in bit 31.  Its far column
# is 46 corners square: at this object's floor (259 x 514 x 13 vertices) one swathe's share fits and two swathes' do not.
K32_SIZE = tuple(min(a, b) for a, b in zip(mk.GRIDS["k32_b"][0], KEYS.dims))
assert K32_SIZE == (260, 513, 257) and mk.layout(K32_SIZE) == (10, 11, 10) and mk.key_bits(K32_SIZE) == 32
K34_STEP = Step("k34", "corner", K34.size, None, "sort", swathes=17, fn=K34.fn)
K32_STEP = Step("k32_clipped", "corner", K32_SIZE, None, "sort", swathes=5, fn=mk.corner_fn(K32_SIZE, 45))
K_SMALL = Step("k_small", "noise", (33, 33, 33), "rows", "lattice")             # a 22-bit layout; one swathe of 64: lattice
KEYS_STEPS = [K32_STEP, K34_STEP, K_SMALL, K34_STEP, K32_STEP]                    # 64 after 32, lattice between, 32 after 64
for _s in KEYS_STEPS:
    assert _s.key_offset == mx.KEY_OFFSET                                         # the oracle run the key tests share

# ---- batches with history: three objects of the wide dims, the sizes rotated from call to call -------------------------------
BATCH_STEPS = [Step("b_nw64", "noise", (2048, 17, 13), "rows", "lattice", overflows=("tight",)),
               Step("b_nw1", "noise", (32, 17, 13), "rows", "lattice"),
               Step("b_tube2049", "tube", (2049, 17, 13), "cells", "lattice")]
BATCH_OFFSETS = [(3 * k, 100 + k, 7 * k) for k in range(3)]


def batch_call(rotation):
    """The steps of lane 0, 1, 2 in call `rotation`: lane k takes size (k + rotation) % 3 with lane k's key offset"""
    out = []
    for k in range(3):
        s = BATCH_STEPS[(k + rotation) % 3]
        out.append(Step(s.name, s.field, s.size, s.route, s.weld, s.swathes, s.overflows, BATCH_OFFSETS[k], s.fn))
    return out


# ---- padding: pitch - width and zStride - height large -------------------------------------------------------------------------
PADDED = Obj("padded", (2056, 24, 24), 24)
PADDED_STEPS = _numbered([Step("p_tube2049", "tube", (2049, 17, 13), "cells", "lattice"),
                          Step("p_nw2", "noise", (33, 5, 4), "rows", "lattice")])

# ---- a failed call in the middle (the deep object) ----------------------------------------------------------------------------
BEYOND = [(68, 35, 264), (67, 36, 264), (67, 35, 265)]                              # one corner beyond the dims, axis by axis
FAILING = Step("d_150", "noise", (65, 33, 150), None, "sort", swathes=3, overflows=("tight",))
AFTER_FAILURE = [DEEP_STEPS[1], DEEP_STEPS[0]]                                     # 65 x 33 x 64, then 65 x 33 x 257

SEQUENCES = {"wide": (WIDE, WIDE_STEPS), "wide_reversed": (WIDE, WIDE_STEPS[::-1]), "deep": (DEEP, DEEP_STEPS),
             "keys": (KEYS, KEYS_STEPS), "padded": (PADDED, PADDED_STEPS)}
MEMORIES = {"wide": ("ample", "tight"), "wide_reversed": ("ample", "tight"), "deep": ("ample", "tight"), "keys": (mk.MEMORY,),
            "padded": ("ample",)}


# ---- the worker ---------------------------------------------------------------------------------------------------------------
WORKER_CLOUD = dict(n=120_000, extent=95.0, spacing=16.0, r_lo=1.5, r_hi=2.5, seed=321)
WORKER_LOW = (40, 40, 40)             # the shells' centre (47.5) lies in every bucket: each of them cuts both shells
WORKER_SIZES = [(64, 64, 64), (9, 64, 17), (64, 9, 9), None, (33, 33, 33), (64, 64, 64)]      # None: a bucket of 0 splats
WORKER_ORDERS = [[(0, 1, 2), (3, 4, 5)], [(4, 2, 1), (5, 3, 0)]]      # every lane sees a size unlike its previous one
WORKER_ORACLE = dict(max_cells=63, max_swathe=64, mesh_memory=63 * 63 * 2 * 872)


def worker_items(num_splats):
    """(first, count, low, num_vertices) of WORKER_SIZES over one resident cloud"""
    return [(0, num_splats, WORKER_LOW, s) if s else (0, 0, WORKER_LOW, (64, 64, 64)) for s in WORKER_SIZES]


@functools.lru_cache(maxsize=None)
def worker_cloud():
    from mlsgpu_amd import synth
    cloud = synth.shells_cloud(**WORKER_CLOUD)
    cloud.setflags(write=False)
    return cloud


@functools.lru_cache(maxsize=None)
def worker_oracle(index):
    """(batches, stats, seconds) of the whole-bucket oracle on item `index` of worker_items alone, on a copy of the cloud"""
    cloud = worker_cloud()
    first, count, low, nv = worker_items(len(cloud))[index]
    t = time.perf_counter()
    batches, st = ob.bucket(cloud.copy(), first, count, nv, low, **WORKER_ORACLE)
    return batches, st, time.perf_counter() - t


# ---- sensitivity: what the step before leaves where the step does not reach ----------------------------------------------------

def sign_changes_outside(field, size):
    """How many neighbouring pairs of corners of `field` [z, y, x] (the step before) change sign with at least one corner
    in the region a step of `size` does not cover, x >= w' or y >= h' or z >= d'; None when that region is empty."""
    D, H, W = field.shape
    w, h, d = size
    outside = np.ones(field.shape, bool)
    outside[:min(d, D), :min(h, H), :min(w, W)] = False
    if not outside.any():
        return None
    neg, ok = field < 0, np.isfinite(field)
    n = 0
    for axis in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        n += int(((neg[a] != neg[b]) & ok[a] & ok[b] & (outside[a] | outside[b])).sum())
    return n


# ---- generators with a poisoned padding ---------------------------------------------------------------------------------------

POISONS = ("nan", "big", "field")


def poison_block(fn, poison, z, width, height, z_stride, pitch):
    """The zStride x pitch block of slice z as a poisoning generator uploads it: the field in [0, height) x [0, width) and
    elsewhere NaN ("nan"), +-3e38 with the sign of the parity of x + y + z so that every neighbouring pair changes sign
    ("big"), or the field function itself evaluated beyond the extent, which is what processCorners leaves there
    ("field")."""
    ys, xs = np.meshgrid(np.arange(z_stride, dtype=np.uint32), np.arange(pitch, dtype=np.uint32), indexing="ij")
    if poison == "nan":
        block = np.full((z_stride, pitch), np.nan, np.float32)
    elif poison == "big":
        block = np.where(((xs + ys + np.uint32(z)) & 1) != 0, np.float32(-3e38), np.float32(3e38)).astype(np.float32)
    else:
        assert poison == "field"
        block = np.ascontiguousarray(fn(xs, ys, z), np.float32)
    block[:height, :width] = np.asarray(fn(xs[:height, :width], ys[:height, :width], z), np.float32)
    return block


class PoisonGenerator:
    """A Marching::Generator like binding.HostGenerator that uploads, for every slice it is asked for, the slice's whole
    zStride x pitch block (poison_block) and nothing outside those blocks.  `obj` bounds what it may write: the blocks of a
    swathe end at row zStride (maxSwathe + 1) of an image of obj.field_rows rows.  fail_at=k makes call k (from 1) of the
    callback raise instead, after which the generator stays failed."""

    def __init__(self, ctx, obj, fn, poison, fail_at=None):
        from mlsgpu_amd import binding as mb
        self.error, self.calls, self.blocks = None, 0, 0

        def enqueue(user, stream, field, pitch, swp):
            try:
                sw = swp.contents
                self.calls += 1
                if fail_at is not None and self.calls >= fail_at:
                    raise GeneratorFailure("call %d" % self.calls)
                assert pitch == obj.pitch and sw.zStride == obj.z_stride
                for z in range(sw.zFirst, sw.zLast + 1):
                    row0 = z * sw.zStride + sw.zBias
                    assert 0 <= row0 and row0 + sw.zStride <= obj.field_rows, (z, row0)
                    block = poison_block(fn, poison, z, sw.width, sw.height, sw.zStride, pitch)
                    mb.check(mb.lib().mlsgpu_hip_memcpy_h2d(ctx.h, field + row0 * pitch * 4, mb._p(block), block.nbytes, 0))
                    self.blocks += 1
                return 0
            except Exception as e:
                # without its traceback: that holds this frame, whose f_back is the frame that made the call -- with the
                # marching object in it -- and self.error closes a cycle, so the object would live until some later
                # collection, possibly past the close of its context (a destroy on a closed context is a use after free)
                self.error = e.with_traceback(None)
                return 5
        self._enqueue = mb.ENQUEUE_FN(enqueue)
        self.struct = mb.Generator()
        for i in range(3):
            self.struct.alignment[i] = mx.ALIGNMENT[i]
        self.struct.enqueue = self._enqueue
        self.struct.user = None


class GeneratorFailure(Exception):
    """What a PoisonGenerator with fail_at raises in its callback"""
