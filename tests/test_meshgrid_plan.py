"""The host arithmetic of the triangle grid (mlsgpu_amd/csrc/meshgridplan.hpp) run without a GPU: a stand-alone driver
(meshgridplan_test.cpp) is built with the address and undefined-behaviour sanitizers and asked, as a child process, what the
grid's plan would decide.  Every answer is worked out again by the numpy model (meshgrid_cases), which is written from the
rule in the header's comment, not from its code.

These figures are the implementation's plan, not part of the deviation or the self-intersection report's contract (both
reports are the same for every cell size); a later tuning change may update the model."""
import os
import struct
import subprocess

import numpy as np
import pytest

import meshgrid_cases as mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlsgpu_amd", "csrc")
CAP = mg.CELL_CAP


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meshgridplan") / "meshgridplan_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(CSRC, "meshgridplan_test.cpp")])
    return exe


def ask(exe, questions):
    """questions: lists of a word and integers; the answers as lists of ints, the word checked"""
    text = "\n".join(" ".join(str(w) for w in q) for q in questions) + "\n"
    done = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert done.returncode == 0, (done.returncode, done.stderr)
    lines = [line.split() for line in done.stdout.splitlines()]
    assert [line[0] for line in lines] == [q[0] for q in questions]
    return [[int(x) for x in line[1:]] for line in lines]


def bits(x):
    """a double as the integer of its bits"""
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def double(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def grid(lo, hi, h, reach=0.0):
    return tuple(bits(x) for x in (*lo, *hi, h, reach))


def lay_expected(lo, hi, h):
    n = mg.lay_grid(lo, hi, h)
    if n is None:
        return [0] * 7
    bx, by = (n[0] - 1).bit_length(), (n[1] - 1).bit_length()
    return [1, *n, bx, bx + by, mg.key_bits(n)]


# ---------------------------------------------------------------------------------------------- layGrid

LAY = {     # lo, hi, h
    "no power of two on any axis": ((0, 0, 0), (10.5, 3.2, 40.0), 1.0),                # 11 x 4 x 41 cells: the shifts matter
    "off the origin": ((-3.25, 7.5, 1e3), (9.0, 7.75, 1e3 + 5), 0.3),
    "a one-point box": ((3, 4, 5), (3, 4, 5), 1.0),
    "a one-point box, a huge cell": ((3, 4, 5), (3, 4, 5), 1e300),
    "exactly the cap": ((0, 0, 0), (CAP - 1, 1, 1), 1.0),                               # floor(CAP - 1) + 1 cells: accepted
    "exactly the cap, its last cell begun": ((0, 0, 0), (CAP - 0.5, 1, 1), 1.0),
    "one cell more": ((0, 0, 0), (CAP, 1, 1), 1.0),
    "one cell more on the last axis": ((0, 0, 0), (1, 1, CAP * 0.25), 0.25),
    "the cap on every axis": ((-1, -1, -1), (CAP - 2, CAP - 2, CAP - 2), 1.0),
    "a NaN cell": ((0, 0, 0), (1, 1, 1), float("nan")),
    "an infinite cell": ((0, 0, 0), (1, 1, 1), float("inf")),                           # one cell: the loop's isfinite leaves first
    "a zero cell": ((0, 0, 0), (1, 1, 1), 0.0),
    "a zero cell over a one-point box": ((2, 2, 2), (2, 2, 2), 0.0),                    # 0 / 0
}


def test_lay_grid(driver):
    got = ask(driver, [("lay",) + grid(*c) for c in LAY.values()])
    by_name = dict(zip(LAY, got))
    for (name, c), g in zip(LAY.items(), got):
        assert g == lay_expected(*c), name
    assert by_name["no power of two on any axis"] == [1, 11, 4, 41, 4, 6, 12]
    assert by_name["a one-point box"] == [1, 1, 1, 1, 0, 0, 0]                          # every n is 1, the key 0 bits wide
    assert by_name["exactly the cap"][:2] == [1, CAP] and by_name["exactly the cap, its last cell begun"][:2] == [1, CAP]
    assert by_name["the cap on every axis"] == [1, CAP, CAP, CAP, 21, 42, 63]
    for name in ("one cell more", "one cell more on the last axis", "a NaN cell", "a zero cell", "a zero cell over a one-point box"):
        assert by_name[name][0] == 0, name
    assert by_name["an infinite cell"] == [1, 1, 1, 1, 0, 0, 0]


# ---------------------------------------------------------------------------------------------- cell()

def test_cell_is_monotone_and_clamped(driver):
    lo, hi, h = (-3.25, 7.5, 0.0), (9.0, 7.75, 5.0), 0.3
    n = mg.lay_grid(lo, hi, h)
    rng = np.random.default_rng(5)
    for axis in range(3):
        x = np.concatenate([rng.uniform(lo[axis] - 3, hi[axis] + 3, 2000), [-0.0, 0.0, lo[axis], hi[axis], lo[axis] - 1e300, hi[axis] + 1e300,
                            np.nextafter(lo[axis], -np.inf), np.nextafter(hi[axis], np.inf), -np.inf, np.inf, 5e-324, -5e-324]])
        x = np.array(sorted(x.tolist()))
        assert (x < lo[axis]).sum() > 5 and (x > hi[axis]).sum() > 5 and np.signbit(x[x == 0]).any()
        x = np.concatenate([x, [np.nan]])
        (got,) = ask(driver, [("cell",) + grid(lo, hi, h) + (axis, len(x)) + tuple(bits(v) for v in x)])
        assert got == mg.cell(lo[axis], h, n[axis], x).tolist()
        assert all(0 <= c <= n[axis] - 1 for c in got)                                  # infinities and the NaN included
        assert (np.diff(got[:-1]) >= 0).all() and got[0] == 0 and got[-2] == n[axis] - 1
        assert len(set(got)) == n[axis]                                                 # every cell of the axis is met


# ---------------------------------------------------------------------------------------------- key / packedOf

def test_key_round_trip(driver):
    cases = [((0, 0, 0), (10.5, 3.2, 40.0), 1.0),                                       # 4, 2 and 6 bits
             ((0, 0, 0), (CAP - 1, 2.0, 300.0), 1.0),                                   # 21, 2 and 9 bits
             ((0, 0, 0), (0.0, 5.0, CAP - 1), 1.0),                                     # 0, 3 and 21 bits
             ((-1, -1, -1), (CAP - 2, CAP - 2, CAP - 2), 1.0)]                          # 63 bits
    questions, want = [], []
    for lo, hi, h in cases:
        n = mg.lay_grid(lo, hi, h)
        bx, by = (n[0] - 1).bit_length(), (n[1] - 1).bit_length()
        for c in ((n[0] - 1, n[1] - 1, n[2] - 1), (0, 0, 0), (n[0] - 1, 0, 0), (0, n[1] - 1, 0), (0, 0, n[2] - 1), (n[0] // 2, n[1] // 3, n[2] // 5)):
            questions.append(("key",) + grid(lo, hi, h) + c)
            want.append([c[2] << (bx + by) | c[1] << bx | c[0], c[2] << 42 | c[1] << 21 | c[0], *c])
    assert ask(driver, questions) == want
    assert max(w[0] for w in want) == (1 << 63) - 1


# ---------------------------------------------------------------------------------------------- firstCellSize, the budget

def test_first_cell_size(driver):
    cases = [   # extentSum, live, eSide, side, reach
        (0, 3, 3, 7.0, 0.0),                    # no reach, every triangle a point: the box's side ...
        (0, 3, 0, 0.0, 0.0),                    # ... or 1, where the box is a point too
        (1, 5, 10, 1000.0, 0.0),                # a mean far below side * 2^-21
        (94322828, 19801, 8, 210.0, 0.0),
        (94322828, 19801, 8, 210.0, 0.25),      # 2 D below the mean: the mean
        (94322828, 19801, 8, 210.0, 0.75),      # 2 D above it: 2 D
        (0, 2, 0, 0.0, 2.0),                    # a one-point target: 2 D
        (4718592, 18, 2, 3.0, 3.0 * 2.0 ** -23),
        ((1 << 21) * 1000, 1000, 1023, 1.5 * 2.0 ** 1022, 0.0)]        # every extent at the clamp, the largest box
    got = ask(driver, [("first", c[0], c[1], c[2], bits(c[3]), bits(c[4])) for c in cases])
    for c, g in zip(cases, got):
        assert double(g[0]) == mg.first_cell_size(*c), c
    values = [double(g[0]) for g in got]
    assert values[:2] == [7.0, 1.0] and values[2] == 2.0 ** -10 / 5 and values[4] == values[3] and values[5] == 1.5 and values[6] == 4.0
    assert values[7] == 1.0 and values[8] == float("inf")                               # which the loop's isfinite refuses


def test_budget(driver):
    lives = [1, 2, (1 << 17) - 1, 1 << 17, (1 << 17) + 1, (1 << 32) // 3]
    assert ask(driver, [("budget", n) for n in lives]) == [[max(1 << 20, 8 * n)] for n in lives]


# ---------------------------------------------------------------------------------------------- the box, the ordered bits

def ordered(f):
    b = int(np.float32(f).view(np.uint32))
    return (~b & 0xFFFFFFFF) if b >> 31 else b | 0x80000000


FLOATS = [-np.inf, -3.4e38, -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.17549435e-38, 0.1, 1.0, 3.4e38, np.inf]


def test_ordered_bits(driver):
    f = np.float32(FLOATS)
    got = ask(driver, [("ordered", int(b)) for b in f.view(np.uint32)])
    assert [g[0] for g in got] == [ordered(x) for x in f]
    assert [g[1] for g in got] == [int(b) for b in f.view(np.uint32)]                   # and back, -0.0 as -0.0
    order = [g[0] for g in got]
    assert all(a < b for a, b in zip(order, order[1:])) and 0 < order[0] and order[-1] < 0xFFFFFFFF


@pytest.mark.parametrize("reach", [0.0, 0.375])
def test_box_of_the_counter_words(driver, reach):
    """The words as the extent kernel leaves them: per axis the largest complement of the ordered bits, and the largest."""
    rng = np.random.default_rng(11)
    meshes = [np.concatenate([rng.uniform(-40, 90, (50, 3)), [[-40, 0, 0], [90, 0, 0]]]).astype(np.float32), np.float32([[3, 4, 5]] * 4), np.float32([[-0.0, 0.0, -1e-45], [0.0, -0.0, 1e-45]]),
              np.float32([[1e-42, 0, 0], [3e-42, 0, 0]]), np.float32([[-3e38, 0, 0], [3e38, 1, 1]])]
    questions = []
    for v in meshes:
        least = [max((~ordered(x)) & 0xFFFFFFFF for x in v[:, k]) for k in range(3)]
        most = [max(ordered(x) for x in v[:, k]) for k in range(3)]
        questions.append(("box", *least, *most, 1, bits(reach)))
    questions.append(("box", 0, 0, 0, 0, 0, 0, 0, bits(reach)))                         # no vertices: the words as they were cleared
    got = ask(driver, questions)
    for v, g in zip(meshes + [np.zeros((0, 3), np.float32)], got):
        lo, hi, side, e_side = mg.box(v, reach)
        if len(v) == 0:
            lo, hi = np.zeros(3), np.zeros(3)                                           # nothing to bin: not inflated either
        assert [double(b) for b in g[:3]] == lo.tolist() and [double(b) for b in g[3:6]] == hi.tolist()
        assert double(g[6]) == side and g[7] == e_side
        if side > 0.0:
            assert 2.0 ** (e_side - 1) <= side < 2.0 ** e_side
    assert [got[k][7] for k in (0, 1, 4, 5)] == [8, 0, 129, 0]                          # 2^7 <= 130 < 2^8; 2^128 <= 6e38 < 2^129
