"""The host arithmetic of marching (mlsgpu_amd/csrc/marchingplan.hpp) run without a GPU: a stand-alone driver
(marchingplan_test.cpp) is built with the address and undefined-behaviour sanitizers and asked, as a child process, what
marching would decide.  Every answer is worked out again here from the reference's rules (src/marching.cpp:273-284 for the
sizes, :627-743 for the slice runs, kernels/marching.cl:148-154 for the half lattice), not from the header."""
import os
import subprocess

import numpy as np
import pytest

import marching_extent_cases as mx
import marching_key_cases as mk
import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlsgpu_amd", "csrc")
MAX_CELL_VERTICES, MAX_CELL_INDICES = 13, 36        # src/marching.h:86-91


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("marchingplan") / "marchingplan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "marchingplan_test.cpp")])
    return exe


def ask(exe, questions):
    """questions: lists of a word and numbers; the answers as lists of ints, the word checked"""
    text = "\n".join(" ".join(str(w) for w in q) for q in questions) + "\n"
    done = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr)
    lines = [line.split() for line in done.stdout.splitlines()]
    assert [line[0] for line in lines] == [q[0] for q in questions]
    return [[int(x) for x in line[1:]] for line in lines]


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------- MarchingSizes

def sizes_expected(W, H, D, limit, memory, a):
    image_w, image_h = ceil_div(W, a[0]) * a[0], ceil_div(H, a[1]) * a[1]
    swathe = min(limit, D) // a[2] * a[2]
    mesh_cells = memory // mx.MAX_CELL_BYTES
    return [image_w, image_h, image_h, swathe, (W - 1) * (H - 1) * swathe, mesh_cells * MAX_CELL_VERTICES,
            mesh_cells * MAX_CELL_INDICES, image_h * (swathe + 1 + a[2]), int(swathe < D),
            (2 * swathe + 1) * (2 * H - 1), ceil_div(2 * W - 1, 64)]


def floor_memory(W, H):
    return (W - 1) * (H - 1) * mx.MAX_CELL_BYTES


# the most mesh cells whose vertices still number less than 2^32, and the last byte that gives no more
ALMOST_2_32 = ((1 << 32) - 1) // MAX_CELL_VERTICES * mx.MAX_CELL_BYTES + mx.MAX_CELL_BYTES - 1

SIZES = [(W, H, D, limit, memory, a)
         for a in [(1, 1, 1), (8, 8, 8), (7, 5, 11)]
         for (W, H, D) in [(35, 11, 24), (2052, 11, 48), (100, 2051, 33)]
         for limit in (D + 9, D, D - 1, 20)             # above, equal to and below maxDepth; 20: 8 and 11 do not divide it
         for memory in (floor_memory(W, H), 7 * floor_memory(W, H) + 123, ALMOST_2_32)]


def test_sizes(driver):
    got = ask(driver, [("sizes",) + c[:5] + c[5] for c in SIZES])
    legacy = set()
    for c, g in zip(SIZES, got):
        assert g == sizes_expected(*c), c
        legacy.add(g[8])
        assert g[3] % c[5][2] == 0 and g[3] <= min(c[3], c[2]) < g[3] + c[5][2]
    assert legacy == {0, 1}
    top = [g for c, g in zip(SIZES, got) if c[4] == ALMOST_2_32]
    assert all((1 << 32) - MAX_CELL_VERTICES <= g[5] < (1 << 32) for g in top)


# ---------------------------------------------------------------------------------------------- LatticeDims

def lattice_expected(W, H, z_top, z_max, rows_max, words_max):
    """the half lattice of cells z in [z_top, z_max): points (x2, y2, z2) = 2 cell + (0..2), x2 <= 2 (W - 1) and so on"""
    nw = ceil_div(2 * (W - 1) + 1, 64)
    layers, rows_per_layer = 2 * (z_max - z_top) + 1, 2 * (H - 1) + 1
    corner_rows = (z_max - z_top + 1) * H
    return [nw, rows_per_layer, 2 * (W - 1), 2 * (H - 1), 2 * z_top, 2 * z_max, W - 1, H - 1, layers * rows_per_layer,
            corner_rows, (z_max - z_top) * (H - 1), layers * rows_per_layer * nw,
            ceil_div(layers, 2) * ceil_div(rows_per_layer, 2),
            ceil_div(corner_rows, 4),                                            # a wave per row of corners, four a workgroup
            ceil_div(corner_rows, 4 * (64 // nw)) if nw <= 64 else 0,            # 64 // nw rows of corners per wave
            int(layers * rows_per_layer <= rows_max and nw <= words_max)]


LATTICE_WIDTHS = {2: 1, 32: 1, 33: 2, 96: 3, 130: 5, 2048: 64, 2049: 65, 8189: 256}


def test_lattice_dims(driver):
    cases = []
    for W, nw in LATTICE_WIDTHS.items():
        assert mx.lattice_words(W) == nw
        for H in (2, 9, 2049):
            for z_top, z_max in ((0, 10), (9, 10), (0, 1), (3, 24)):
                rows = (2 * (z_max - z_top) + 1) * (2 * H - 1)
                for rows_max, words_max in ((rows, nw), (rows - 1, nw), (rows + 1, nw), (rows, nw - 1), (1 << 40, 256)):
                    cases.append((W, H, z_top, z_max, rows_max, words_max))
    got = ask(driver, [("lattice",) + c for c in cases])
    for c, g in zip(cases, got):
        assert g == lattice_expected(*c), c
    fits = [g[15] for g in got]
    assert fits.count(1) == 3 * len(fits) // 5 and fits[0::5] == [1] * (len(fits) // 5)
    # idle lanes in the word kernel's wave: 21 rows of corners a wave at nw 3, 12 at nw 5
    by_words = {c[0]: g[14] for c, g in zip(cases, got) if c[1:4] == (9, 0, 10)}
    assert by_words[96] == ceil_div(11 * 9, 4 * 21) and by_words[130] == ceil_div(11 * 9, 4 * 12)
    assert by_words[2048] == ceil_div(11 * 9, 4) and by_words[2049] == 0


# ---------------------------------------------------------------------------------------------- the route rules

def test_mask_by_rows(driver):
    cases = [(nw, forced) for nw in (1, 3, 5, 63, 64, 65, 256) for forced in (0, 1)]
    got = ask(driver, [("mask",) + c for c in cases])
    assert [g[0] for g in got] == [int(forced == 1 or nw > 64) for nw, forced in cases]


def test_triangles_by_cells(driver):
    cases = []
    for nw in (1, 64, 65):
        for cell_rows, cw in ((8 * 9, 31), (16 * 12, 100), (3, 4), (65535 * 7, 8188)):
            cells = cell_rows * cw
            for occupied in {cells // 4 - 1, cells // 4, cells // 4 + 1, ceil_div(cells, 4), ceil_div(cells, 4) - 1, 1, cells}:
                for forced in (-1, 0, 1):
                    cases.append((nw, occupied, cell_rows, cw, forced))
    got = ask(driver, [("triangles",) + c for c in cases])
    seen = set()
    for (nw, occupied, cell_rows, cw, forced), g in zip(cases, got):
        # by rows when at least a quarter of the cells are occupied; the override rules below 65 words, above nothing does
        rule = 4 * occupied < cell_rows * cw
        want = True if nw > 64 else (rule if forced < 0 else forced == 1)
        assert g == [int(want)], (nw, occupied, cell_rows, cw, forced)
        seen.add((nw > 64, forced, rule))
    assert len(seen) == 12
    exact = [g[0] for c, g in zip(cases, got) if c == (64, 16 * 12 * 100 // 4, 16 * 12, 100, -1)]
    assert exact == [0]                                 # exactly a quarter: by rows


def test_weld_route(driver):
    LATTICE, SORT, NONE = 0, 1, 2
    cases = {(10, 24, 0, 0): LATTICE, (24, 24, 1, 0): LATTICE, (25, 24, 1, 0): SORT,       # several swathes
             (10, 24, 1, 1): SORT,                                                         # forced, and the buffers exist
             (10, 24, 0, 1): LATTICE,                                                      # forced without them: ignored
             (25, 24, 0, 0): NONE, (25, 24, 0, 1): NONE, (25, 24, 1, 1): SORT}
    got = ask(driver, [("weld",) + c for c in cases])
    assert [g[0] for g in got] == list(cases.values())
    assert set(cases.values()) == {LATTICE, SORT, NONE}


def test_key_layout(driver):
    sizes = [mk.GRIDS[n][0] for n in mk.NAMES] + [(2, 2, 2), (3, 2, 1), (8192, 8192, 8192)]
    got = ask(driver, [("keys",) + tuple(s) for s in sizes])
    for s, g in zip(sizes, got):
        want = [(2 * (n - 1)).bit_length() or 1 for n in s]       # bits of the largest doubled local coordinate, at least one
        assert g == want + [sum(want) + 1, int(sum(want) + 1 > 32)], s
    bits = {n: g[3] for n, g in zip(mk.NAMES, got)}
    assert bits == {n: mk.GRIDS[n][1] for n in mk.NAMES} and set(bits.values()) == {31, 32, 33, 34}


# ---------------------------------------------------------------------------------------------- sliceRun

def run_expected(hist, first, last, offsets, space):
    """src/marching.cpp:661-685"""
    sub_last, counts = first, [0, 0]
    while sub_last < last and all(offsets[j] + counts[j] + hist[sub_last][j] <= space[j] for j in range(2)):
        counts = [counts[j] + hist[sub_last][j] for j in range(2)]
        sub_last += 1
    if sub_last == first:
        while sub_last < last and all(counts[j] + hist[sub_last][j] <= space[j] for j in range(2)):
            counts = [counts[j] + hist[sub_last][j] for j in range(2)]
            sub_last += 1
    return sub_last


def run_question(hist, first, last, offsets, space):
    """the driver gets the slices below `last` and no more: a read behind them is the sanitizer's to report"""
    return ("run", first, last, *offsets, *space, last, *[v for h in hist[:last] for v in h])


RUNS = {    # hist, first, last, offsets, (vertexSpace, indexSpace): end
    "everything fits": ([(10, 30)] * 5, 0, 5, (0, 0), (100, 300), 5),
    "from the middle": ([(10, 30)] * 5, 2, 5, (5, 5), (100, 300), 5),
    "only after a flush": ([(60, 90), (50, 90), (30, 90)], 0, 3, (50, 0), (100, 300), 1),
    "after a flush, two": ([(60, 90), (30, 90), (30, 90)], 0, 3, (50, 200), (100, 300), 2),
    "exactly the vertex space": ([(40, 3), (60, 3), (1, 3)], 0, 3, (0, 0), (100, 300), 2),
    "exactly, behind what is buffered": ([(40, 3), (50, 3), (1, 3)], 0, 3, (10, 0), (100, 300), 2),
    "one more vertex": ([(40, 3), (61, 3), (1, 3)], 0, 3, (0, 0), (100, 300), 1),
    "limited by indices": ([(1, 100), (1, 100), (1, 100), (1, 1)], 0, 4, (0, 0), (100, 300), 3),
    "exactly the index space, buffered": ([(1, 100), (1, 100), (1, 1)], 0, 3, (0, 100), (100, 300), 2),
    "a slice too big": ([(101, 3), (1, 3)], 0, 2, (0, 0), (100, 300), 0),
    "a slice too big, by indices, later": ([(1, 3), (1, 301)], 1, 2, (7, 7), (100, 300), 1),
    "empty range": ([(1, 3), (1, 3)], 1, 1, (0, 0), (100, 300), 1),
    "no slices at all": ([], 0, 0, (5, 5), (100, 300), 0),
    "above 2^32 together": ([((1 << 32) - 2, 6), (5, 6)], 0, 2, ((1 << 32) - 10, 0), ((1 << 32) - 1, 300), 1),
}


def test_slice_runs(driver):
    got = ask(driver, [run_question(*c[:5]) for c in RUNS.values()])
    for (name, c), g in zip(RUNS.items(), got):
        assert run_expected(*c[:5]) == c[5], name           # the table against the reference's loops
        assert g == [c[5]], name


def slice_histogram(case):
    """(vertices, indices) of every slice of cells of a case, from its field and the reference's tables"""
    count = ob.make_tables()[0]
    field = mx.field_array(case.fn, case.size)
    D, H, W = field.shape
    code = np.zeros((D - 1, H - 1, W - 1), np.uint32)
    valid = np.ones(code.shape, bool)
    for i in range(8):
        corner = field[(i >> 2):(i >> 2) + D - 1, ((i >> 1) & 1):((i >> 1) & 1) + H - 1, (i & 1):(i & 1) + W - 1]
        code |= (corner >= 0).astype(np.uint32) << np.uint32(i)
        valid &= np.isfinite(corner)
    code = np.where(valid & (code != 255), code, 0)
    per_cell = count[code].astype(np.int64)                 # code 0: no vertices, no indices
    return [tuple(int(v) for v in per_cell[z].sum(axis=(0, 1))) for z in range(D - 1)]


def split_as_add_slices(driver, hist, space):
    """Marching::generate for a bucket of one swathe with sliceRun as its splitter: the ship-outs as (zTop, zMax, vertices,
    indices) and the number of overflows.  Offsets are reset at each flush."""
    state = dict(offsets=[0, 0], z_top=0, ships=[], overflows=0)

    def ship_out(z_max):
        state["ships"].append((state["z_top"], z_max, *state["offsets"]))
        state["offsets"] = [0, 0]

    def add_slices(first, last):
        counts = [sum(h[j] for h in hist[first:last]) for j in range(2)]
        if counts[0] == 0:
            return
        if counts[0] > space[0] or counts[1] > space[1]:
            state["overflows"] += 1
            sub_first = first
            while sub_first < last:
                ((sub_last,),) = ask(driver, [run_question(hist, sub_first, last, state["offsets"], space)])
                assert sub_last == run_expected(hist, sub_first, last, state["offsets"], space) and sub_last > sub_first
                add_slices(sub_first, sub_last)
                sub_first = sub_last
        else:
            if any(state["offsets"][j] + counts[j] > space[j] for j in range(2)):
                ship_out(first)
                state["z_top"] = first
            state["offsets"] = [state["offsets"][j] + counts[j] for j in range(2)]

    add_slices(0, len(hist))
    if state["offsets"][0] > 0:
        ship_out(len(hist))
    return state["ships"], state["overflows"]


@pytest.mark.parametrize("field,width", [("noise", 32), ("noise", 96), ("tube", 33)])
def test_whole_split_equals_the_oracle(driver, field, width):
    """A bucket at tight mesh memory (two slices of maximum cells): the runs sliceRun cuts are the oracle's ship-outs"""
    case = mx.width_case(field, width)
    batches, stats = mx.oracle_run(case, "tight")
    hist = slice_histogram(case)
    memory = case.memory("tight")
    (sizes,) = ask(driver, [("sizes",) + case.dims + (case.swathe, memory) + mx.ALIGNMENT])
    space = (sizes[5], sizes[6])
    ships, overflows = split_as_add_slices(driver, hist, space)
    assert sum(s[2] for s in ships) == stats["unwelded"] and sum(s[3] for s in ships) == stats["indices"]
    assert (len(ships), overflows) == (stats["shipouts"], stats["overflows"])
    assert [s[3] // 3 for s in ships] == [len(b["triangles"]) for b in batches]
    # the ship-outs' slices follow each other and cover the bucket's surface
    assert all(a[1] == b[0] for a, b in zip(ships, ships[1:])) and all(s[2] <= space[0] and s[3] <= space[1] for s in ships)
    if field == "noise":
        assert overflows == 1 and len(ships) >= 3
