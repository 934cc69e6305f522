"""The host arithmetic of one bucketing level (mlsgpu_amd/csrc/bucketplan.hpp), which both routes of the device bucketer
share, run without a GPU: a stand-alone driver (bucketplan_test.cpp) is built with the address and undefined-behaviour
sanitizers and asked, as a child process, what it plans for a case."""
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from bucket_checks import random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlsgpu_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bucketplan") / "bucketplan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "bucketplan_test.cpp")])
    return exe


def run(exe, dims, lo, n, p, counts=None):
    """counts: per chunk (x-major) a list of [z, y, x] arrays, finest level first"""
    words = [*dims, *lo, n, p["max_splats"], p["max_cells"], p["max_split"], p["chunk_cells"], p["micro_cells"],
             0 if counts is None else 1]
    for chunk in counts or []:
        for level in chunk:
            words.extend(int(v) for v in level.ravel())
    done = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    plan, chunks = None, []
    for line in done.stdout.splitlines():
        kind, *v = line.split()
        v = [int(x) for x in v]
        if kind == "plan":
            plan = dict(micro=v[0], chunk_cells=v[1], chunks=v[2:5], levels=v[5], ratio=v[6], ok=v[7])
        elif kind == "chunk":
            chunks.append(dict(cc=v[0:3], lo=v[3:6], hi=v[6:9], dims=v[9:12], bias=v[12:15], total=v[15], n0=v[16], ok=v[17],
                               levels=[], regions=[], table=None))
        elif kind == "level":
            assert v[0] == len(chunks[-1]["levels"])
            chunks[-1]["levels"].append(dict(dims=v[1:4], offset=v[4]))
        elif kind == "picked":
            chunks[-1]["picked"] = (v[0], v[1])
        elif kind == "region":
            chunks[-1]["regions"].append(dict(c=tuple(v[0:3]), level=v[3], count=v[4], lo=v[5:8], hi=v[8:11]))
        else:
            assert kind == "table"
            chunks[-1]["table"] = v
    return plan, chunks


def ceil_div(a, b):
    return -(-a // b)


def check_plan(plan, chunks, dims, lo, n, p):
    """the properties of a level's geometry, and every chunk's layout worked out again"""
    assert plan["ok"] == 1
    m = p["micro_cells"]
    if m == 0 or m > max(dims):
        m = ob.lib().orc_choose_micro_size(ob._p(np.asarray(dims, np.uint32)), p["max_split"], n, p["max_splats"], p["max_cells"])
    while np.prod([ceil_div(d, m) for d in dims], dtype=object) > p["max_split"]:
        m *= 2
    assert plan["micro"] == m
    cells = plan["chunk_cells"]
    assert cells % m == 0 and plan["ratio"] == cells // m
    assert cells >= min(max(dims), p["chunk_cells"] or max(dims))      # never less than asked for, or than the grid needs
    assert plan["chunks"] == [ceil_div(d, cells) for d in dims]
    levels = plan["levels"]
    assert (m << (levels - 1)) >= cells and (levels == 1 or (m << (levels - 2)) < cells)
    # the chunks tile the grid exactly, x-major
    expect = [(x, y, z) for x in range(plan["chunks"][0]) for y in range(plan["chunks"][1]) for z in range(plan["chunks"][2])]
    assert [tuple(c["cc"]) for c in chunks] == expect
    covered = 0
    for c in chunks:
        assert c["ok"] == 1
        for a in range(3):
            assert c["lo"][a] == lo[a] + c["cc"][a] * cells
            assert c["hi"][a] == min(c["lo"][a] + cells, lo[a] + dims[a]) and c["hi"][a] > c["lo"][a]
            assert c["dims"][a] == ceil_div(c["hi"][a] - c["lo"][a], m)
            assert c["bias"][a] == c["cc"][a] * plan["ratio"]
        covered += int(np.prod([c["hi"][a] - c["lo"][a] for a in range(3)], dtype=object))
        offset = 0
        assert len(c["levels"]) == levels
        for l, level in enumerate(c["levels"]):
            assert level["dims"] == [ceil_div(d, 1 << l) for d in c["dims"]] and level["offset"] == offset
            offset += int(np.prod(level["dims"]))
        assert c["total"] == offset and c["n0"] == int(np.prod(c["dims"]))
    assert covered == int(np.prod(dims, dtype=object))


HAND = [dict(max_splats=12_000, max_cells=63, chunk_cells=40, micro_cells=8, max_split=1 << 20),
        dict(max_splats=12_000, max_cells=63, chunk_cells=57, micro_cells=19, max_split=64)]


@pytest.mark.parametrize("seed", range(12))
def test_plan_of_random_cases(driver, seed):
    splats, grid, p = random_case(seed)
    ext = grid["extents"]
    dims = [int(ext[2 * a + 1] - ext[2 * a]) for a in range(3)]
    lo = [int(ext[2 * a]) for a in range(3)]
    plan, chunks = run(driver, dims, lo, len(splats), p)
    check_plan(plan, chunks, dims, lo, len(splats), p)


@pytest.mark.parametrize("p,micro,cells,per_axis,levels", [(HAND[0], 8, 40, 3, 4), (HAND[1], 38, 76, 2, 2)])
def test_plan_of_hand_cases(driver, p, micro, cells, per_axis, levels):
    dims, lo = [114, 114, 114], [-63, 0, 63]
    plan, chunks = run(driver, dims, lo, 150_000, p)
    check_plan(plan, chunks, dims, lo, 150_000, p)
    assert (plan["micro"], plan["chunk_cells"], plan["chunks"], plan["levels"]) == (micro, cells, [per_axis] * 3, levels)


def test_plan_refuses_more_levels_than_the_layout_holds(driver):
    """2^31 + 1 microblocks of one cell along x need 33 octree levels: the caller turns this into a length error"""
    p = dict(max_splats=10, max_cells=(1 << 32) - 1, chunk_cells=0, micro_cells=1, max_split=1 << 63)
    plan, chunks = run(driver, [(1 << 31) + 1, 1, 1], [-(1 << 31), 0, 0], 100, p)
    assert (plan["micro"], plan["levels"], plan["ok"]) == (1, 33, 0) and chunks == []


def box_counters(rng, dims, levels, boxes):
    """counters of `boxes` random boxes of at most two microblocks per axis: a node counts the boxes that touch it"""
    lo = rng.integers(0, dims, (boxes, 3))
    hi = np.minimum(lo + rng.integers(0, 2, (boxes, 3)), np.asarray(dims) - 1)
    out = []
    for l in range(levels):
        d = [ceil_div(v, 1 << l) for v in dims]
        c = np.zeros((d[2], d[1], d[0]), np.uint32)
        for a, b in zip(lo >> l, hi >> l):
            c[a[2]:b[2] + 1, a[1]:b[1] + 1, a[0]:b[0] + 1] += 1
        out.append(c)
    return out


def pick_nodes(counts, dims, micro, max_cells, max_splats):
    """pickNodes as the reference writes it: recursive, child 0 first, x fastest"""
    regions = []

    def visit(c, level):
        count = int(counts[level][c[2], c[1], c[0]])
        if count == 0:
            return
        if level == 0 or ((micro << level) <= max_cells and count <= max_splats):
            regions.append((c, level, count))
            return
        for idx in range(8):
            child = (2 * c[0] + (idx & 1), 2 * c[1] + ((idx >> 1) & 1), 2 * c[2] + (idx >> 2))
            if all((child[a] << (level - 1)) < dims[a] for a in range(3)):
                visit(child, level - 1)
    visit((0, 0, 0), len(counts) - 1)
    return regions


PICK = [  # microblocks of the grid, expected levels, parameters: microblocks of 2 cells, regions of up to 8
    ((1, 1, 1), 1, dict(max_splats=6, max_cells=8, chunk_cells=0, micro_cells=2, max_split=1 << 20), 2),
    ((3, 3, 3), 3, dict(max_splats=6, max_cells=8, chunk_cells=0, micro_cells=2, max_split=1 << 20), 2),
    ((5, 5, 5), 4, dict(max_splats=6, max_cells=8, chunk_cells=0, micro_cells=2, max_split=1 << 20), 2),
    ((7, 2, 1), 4, dict(max_splats=6, max_cells=8, chunk_cells=0, micro_cells=2, max_split=1 << 20), 2),
    (None, 4, dict(HAND[0], max_splats=9), 8),      # 27 chunks of 5^3 microblocks: the root may never be a region
    (None, 2, dict(HAND[1], max_splats=9), 38),     # 8 chunks of 2^3
]


@pytest.mark.parametrize("case", range(len(PICK)))
@pytest.mark.parametrize("boxes", [3, 40])
def test_pick_regions(driver, case, boxes):
    blocks, levels, p, micro = PICK[case]
    dims = [114, 114, 114] if blocks is None else [b * micro for b in blocks]
    lo = [-5, 3, 0]
    rng = np.random.default_rng(500 + 10 * case + boxes)
    layout, chunks = run(driver, dims, lo, 1000, p)
    assert layout["levels"] == levels and layout["micro"] == micro
    if blocks is not None:
        assert len(chunks) == 1 and tuple(chunks[0]["dims"]) == blocks
    counts = [box_counters(rng, c["dims"], levels, boxes) for c in chunks]
    plan, chunks = run(driver, dims, lo, 1000, p, counts)
    check_plan(plan, chunks, dims, lo, 1000, p)
    seen_levels = set()
    for c, cnt in zip(chunks, counts):
        d = c["dims"]
        want = pick_nodes(cnt, d, micro, p["max_cells"], p["max_splats"])
        assert c["picked"] == (1, len(want))
        assert [(r["c"], r["level"], r["count"]) for r in c["regions"]] == want
        # every non-empty microblock lies in exactly one region, and the table says which
        owner = np.full((d[2], d[1], d[0]), -1, np.int64)
        for i, r in enumerate(c["regions"]):
            x, l = r["c"], r["level"]
            cut = owner[x[2] << l:(x[2] + 1) << l, x[1] << l:(x[1] + 1) << l, x[0] << l:(x[0] + 1) << l]
            assert cut.size > 0 and (cut == -1).all()
            cut[...] = (i << 5) | l
            seen_levels.add(l)
            # within both limits above level 0; the parent (which was split) misses one
            if l > 0:
                assert (micro << l) <= p["max_cells"] and r["count"] <= p["max_splats"]
            if l + 1 < levels:
                parent = int(cnt[l + 1][x[2] >> 1, x[1] >> 1, x[0] >> 1])
                assert (micro << (l + 1)) > p["max_cells"] or parent > p["max_splats"]
            # the child box: the node's cells, inside the chunk
            for a in range(3):
                assert r["lo"][a] == min(c["lo"][a] + ((micro * x[a]) << l), c["hi"][a])
                assert r["hi"][a] == min(c["lo"][a] + ((micro * (x[a] + 1)) << l), c["hi"][a])
                assert c["lo"][a] <= r["lo"][a] < r["hi"][a] <= c["hi"][a]
        assert (owner[cnt[0] > 0] >= 0).all()       # (regions do not overlap: checked as they were entered)
        np.testing.assert_array_equal(np.asarray(c["table"], np.int64), np.where(owner >= 0, owner, 0).ravel())
    if boxes == 40 and case in (1, 2, 4):
        assert len(seen_levels) >= 2        # these cases do split, and do keep whole nodes
