"""The layout of the stepper's profile table and the fill of one per-timestep image of it (xlb_amd/csrc/prof_table.hpp) compiled
for the CPU.  The table is the merge of the static entries and the time-dependent cells, sorted by storage cell; td_pos is the
row of every time-dependent cell in DECLARATION order; `contiguous` says td_pos[i] == td_pos[0] + i, i.e. a timestep's values go
in as one block.  Expected values, worked by hand:

  case  static keys  time-dependent  sorted keys          td_pos   contiguous
  1     5, 9, 40     20, 21, 22      5 9 20 21 22 40      2 3 4    yes
  2     9, 20        30, 7           7 9 20 30            3 0      no
  3     8            7, 9            7 8 9                0 2      no  (a static row in between)
  4     -            22, 21          21 22                1 0      no  (rows adjacent, but not in declaration order)
  5     5 twice                      5                                 the later values, one row

Case 6 fills an image: the rows at td_pos hold (T)value of the timestep's values — 0.1 and 1/3 are exact in neither type, so the
fp32 image holds their fp32 roundings (struct's "<f") — and every other row keeps the bytes of its static values."""

import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("prof_table") / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "prof_table_driver.cpp"), "-o", str(exe)], check=True, timeout=300)
    return lambda lines: subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()


def declare(static, td):
    return [f"static {k} {k}.5 {k}.25 {k}.125" for k in static] + [f"td {k}" for k in td]


@pytest.mark.parametrize(
    "static, td, keys, td_pos, contiguous",
    [
        ([5, 9, 40], [20, 21, 22], "5 9 20 21 22 40", "2 3 4", 1),
        ([9, 20], [30, 7], "7 9 20 30", "3 0", 0),
        ([8], [7, 9], "7 8 9", "0 2", 0),
        ([], [22, 21], "21 22", "1 0", 0),
    ],
)
def test_sorted_table_and_the_rows_of_the_time_dependent_cells(driver, static, td, keys, td_pos, contiguous):
    cmds = declare(static, td)
    got = driver(cmds + ["layout", "values"])
    assert got[: len(cmds)] == ["ok"] * len(cmds)
    assert got[len(cmds)] == f"keys {keys} | td_pos {td_pos} | contiguous {contiguous}"
    # values follow their keys: k.5 k.25 k.125 for a static cell, the placeholder zeros for a time-dependent one
    exp = []
    for k in map(int, keys.split()):
        exp += [0.0, 0.0, 0.0] if k in td else [k + 0.5, k + 0.25, k + 0.125]
    assert [float(v) for v in got[len(cmds) + 1].split()] == exp


def test_the_order_of_declaration_among_static_entries_does_not_matter(driver):
    a = driver(declare([40, 5, 9], [20, 21, 22]) + ["layout", "values"])[-2:]
    b = driver(declare([5, 9, 40], [20, 21, 22]) + ["layout", "values"])[-2:]
    assert a == b and a[0] == "keys 5 9 20 21 22 40 | td_pos 2 3 4 | contiguous 1"


def test_a_static_entry_written_twice_keeps_the_later_values(driver):
    got = driver(["static 5 1 2 3", "static 5 4 5 6", "layout", "values"])
    assert got[2] == "keys 5 | td_pos | contiguous 1"
    assert got[3] == "4 5 6"


def test_a_table_without_time_dependent_cells_fills_nothing(driver):
    got = driver(declare([5, 9], []) + ["fill f64 auto", "fill f64 cells"])
    exp = " ".join(struct.pack("<d", v).hex() for k in (5, 9) for v in (k + 0.5, k + 0.25, k + 0.125))
    assert got[2:] == [exp, exp]


STEP = [0.1, 1 / 3, -0.1, 2 / 3, 0.7, 1e-3, -1 / 3, 0.3, 1.1]  # [3 cells][3], none exact in fp32 (or fp64)


@pytest.mark.parametrize("type_, fmt", [("f32", "<f"), ("f64", "<d")])
def test_fill_converts_to_the_image_type_and_leaves_the_static_rows(driver, type_, fmt):
    # case 1: rows 2, 3, 4 take the timestep's values in declaration order; rows 0, 1, 5 keep the static cells 5, 9, 40
    vals = " ".join(repr(v) for v in STEP)
    got = driver(declare([5, 9, 40], [20, 21, 22]) + [f"fill {type_} auto {vals}", f"fill {type_} block {vals}", f"fill {type_} cells {vals}"])[6:]
    static = lambda k: [k + 0.5, k + 0.25, k + 0.125]
    exp = " ".join(struct.pack(fmt, v).hex() for v in static(5) + static(9) + STEP + static(40))
    assert got[0] == exp
    assert got[1] == exp and got[2] == exp  # the block path and the per-cell path leave the same bytes


@pytest.mark.parametrize("type_, fmt", [("f32", "<f"), ("f64", "<d")])
def test_fill_of_scattered_rows_follows_declaration_order(driver, type_, fmt):
    # case 2: cells 30, 7 declared in that order sit in the rows 3 and 0; the static cells 9 and 20 in the rows 1 and 2
    step = STEP[:6]
    vals = " ".join(repr(v) for v in step)
    got = driver(declare([9, 20], [30, 7]) + [f"fill {type_} auto {vals}", f"fill {type_} block {vals}"])[4:]
    exp = step[3:6] + [9.5, 9.25, 9.125] + [20.5, 20.25, 20.125] + step[0:3]
    assert got[0] == " ".join(struct.pack(fmt, v).hex() for v in exp)
    assert got[1] == "bad fill"  # (the driver refuses the block path for rows that are no block)
