"""The steppers' descriptor parser (xlb_amd/csrc/bc_tables.hpp) and the block shape of the row kernels (xlb_amd/csrc/launch_shape.hpp)
compiled for the CPU.  Expected values, worked by hand:

Parser, q = 9, descriptors (id 1 equilibrium = kind 1), (id 2 halfway = kind 2, values[3] = 0.05, values[10] = 0.7), (id 7 do-nothing
= kind 4), in this order:
  ids_packed    one id per byte, first descriptor lowest: 0x07 << 16 | 0x02 << 8 | 0x01           = 0x070201
  kinds_packed  one kind per nibble:                      4 << 8 | 2 << 4 | 1                      = 0x421
  moving_mask   bit i: descriptor i is a halfway wall with a non-zero value among its first q: bit 1 = 0b010
  needs_missing halfway reads the missing mask: 1;  extended_bcs: no kind >= 5: 0;  has_outflow: no kind 9: 0
  has_edge_kinds do-nothing is none of the two-step kernel's: 1
  vals[2]       slot 3 = 0.05; slot 10 is beyond q = 9 and is NOT copied: 0
Ten fullway walls (kind 3) with ids 11..20, the ninth a halfway wall with a moving term instead: the packed words hold the first
eight only: ids 0x1211100f0e0d0c0b, kinds 0x33333333, moving_mask 0 — and kind[19] = 2, kind[20] = 3 are in the table all the same.

Block shape: threads along z tz = nzq when a row fits the block, else the row in ceil(nzq / threads) equal chunks rounded up to whole
waves of 64 (and at most `threads`); block_tz > 0 narrows tz; ty = threads // tz rows (at least 1, at most ny);
grid = (ceil(nzq / tz), ceil(ny / ty), planes):
  nzq  ny planes threads block_tz   tz  ty   grid
   16  16   4     256     0         16  16   1 1 4
   64   3   1     256     0         64   3   1 1 1   ty = 4 capped by ny
  384   8   2     256     0        192   1   2 8 2   2 chunks of 192
  320   3   1     256     0        192   1   2 3 1   2 chunks of 160 -> 192: the second block of a row is part-empty
  384   8   2     256    64         64   4   6 2 2   block_tz narrows 192 to 64
  300   5   1     128     0        128   1   3 5 1   3 chunks of 100 -> 128
   32  30   3     256    16         16  16   2 2 3   (tests/_step_matrix.py: (3, 30, 128) vec 4 block_tz 16)
   32  30   3     128    16         16   8   2 4 3
  257   1   1     256     0        192   1   2 1 1   2 chunks of 129 -> 192
 1000   2   1     256     0        256   1   4 2 1   4 chunks of 250 -> 256
  100   7   2      64     0         64   1   2 7 2   2 chunks of 50 -> 64"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EQUILIBRIUM, HALFWAY, FULLWAY, DO_NOTHING, ZOUHE_VELOCITY, OUTFLOW, HYBRID_FIRST, HYBRID_LAST, HALFWAY_PROFILE = 1, 2, 3, 4, 5, 9, 10, 12, 13


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("bc_tables") / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "bc_tables_driver.cpp"), "-o", str(exe)], check=True, timeout=300)
    return lambda lines: subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()


THREE = "1:1 2:2:3=0.05:10=0.7 7:4"


@pytest.mark.parametrize("who", ["stepper", "scalar", "adjoint"])
def test_three_conditions_on_d2q9(driver, who):
    got = driver([f"parse {who} 9 {THREE}", "kind 1", "kind 2", "kind 7", "kind 3", "vals 2", "vals 1"])
    assert got[0] == "ids 70201 kinds 421 moving 2 needs_missing 1 extended_bcs 0 has_outflow 0 has_edge_kinds 1"
    assert got[1:5] == ["1", "2", "4", "0"]
    vals = [float(v) for v in got[5].split()]
    assert vals[3] == 0.05 and vals[:3] == [0.0] * 3 and vals[4:9] == [0.0] * 5
    assert vals[9:] == [0.0] * 18  # only q values are copied: the descriptor's slot 10 holds 0.7
    assert [float(v) for v in got[6].split()] == [0.0] * 27


def test_a_value_beyond_q_moves_no_wall(driver):
    # the halfway wall's only non-zero value sits in slot 10: within q = 19 it is a moving-wall term, beyond q = 9 it is nothing
    assert driver(["parse stepper 9 2:2:10=0.7"])[0].split()[5] == "0"
    got = driver(["parse stepper 19 2:2:10=0.7", "vals 2"])
    assert got[0].split()[5] == "1" and float(got[1].split()[10]) == 0.7


def test_the_ninth_and_tenth_condition_stay_out_of_the_packed_words(driver):
    bcs = " ".join(f"{11 + i}:{HALFWAY if i == 8 else FULLWAY}" + (":0=0.1" if i == 8 else "") for i in range(10))
    got = driver([f"parse stepper 19 {bcs}", "kind 19", "kind 20"])
    assert got[0] == "ids 1211100f0e0d0c0b kinds 33333333 moving 0 needs_missing 1 extended_bcs 0 has_outflow 0 has_edge_kinds 0"
    assert got[1:] == ["2", "3"]


def test_flags_of_the_extended_kinds(driver):
    # Zou-He velocity (kind 5): extended, reads the missing mask, an edge kind; outflow (kind 9) adds has_outflow
    assert driver([f"parse stepper 19 4:{ZOUHE_VELOCITY}"])[0] == "ids 4 kinds 5 moving 0 needs_missing 1 extended_bcs 1 has_outflow 0 has_edge_kinds 1"
    assert driver([f"parse stepper 19 4:{OUTFLOW} 5:{FULLWAY}"])[0] == "ids 504 kinds 39 moving 0 needs_missing 1 extended_bcs 1 has_outflow 1 has_edge_kinds 1"
    assert driver(["parse stepper 19 5:3"])[0] == "ids 5 kinds 3 moving 0 needs_missing 0 extended_bcs 0 has_outflow 0 has_edge_kinds 0"
    assert driver(["parse stepper 19"])[0] == "ids 0 kinds 0 moving 0 needs_missing 0 extended_bcs 0 has_outflow 0 has_edge_kinds 0"


@pytest.mark.parametrize("who", ["stepper", "scalar", "adjoint"])
def test_bad_ids_are_refused_with_the_library_s_messages(driver, who):
    assert driver([f"parse {who} 9 0:1"]) == ["error bc id 0 out of range 1..255"]
    assert driver([f"parse {who} 9 1:1 256:1"]) == ["error bc id 256 out of range 1..255"]
    assert driver([f"parse {who} 9 -3:1"]) == ["error bc id -3 out of range 1..255"]
    assert driver([f"parse {who} 9 3:1 4:2 3:3"]) == ["error bc id 3 used twice"]
    assert driver([f"parse {who} 9 255:1"])[0].startswith("ids ff ")


@pytest.mark.parametrize("kind", [HYBRID_FIRST, 11, HYBRID_LAST])
def test_who_takes_a_hybrid_kind(driver, kind):
    for q in (9, 19, 27):
        assert driver([f"parse scalar {q} 1:{kind}"]) == [f"error refused kind {kind}"]
        assert driver([f"parse adjoint {q} 1:{kind}"]) == [f"error refused kind {kind}"]
    assert driver([f"parse stepper 9 1:{kind}"]) == ["error This BC is not implemented in 2D!"]
    for q in (19, 27):
        assert driver([f"parse stepper {q} 1:{kind}", "kind 1"]) == [f"ids 1 kinds {kind:x} moving 0 needs_missing 1 extended_bcs 1 has_outflow 0 has_edge_kinds 1", str(kind)]


def test_the_other_acceptance_rules(driver):
    # the stepper: kinds 1..13; the scalar step: the basic kinds, the Zou-He family and the outflow; the adjoint: the basic kinds
    for kind in (0, 14, -1):
        assert driver([f"parse stepper 19 1:{kind}"]) == [f"error unknown bc kind {kind}"]
    for kind in range(1, 14):
        assert driver([f"parse stepper 19 1:{kind}"])[0].startswith("ids 1 ")
        assert driver([f"parse scalar 19 1:{kind}"])[0].startswith("ids 1 " if kind <= 9 else "error refused")
        assert driver([f"parse adjoint 19 1:{kind}"])[0].startswith("ids 1 " if kind <= 4 else "error refused")
    assert driver([f"parse scalar 19 1:{HALFWAY_PROFILE}"]) == [f"error refused kind {HALFWAY_PROFILE}"]
    assert driver(["parse scalar 19 1:0"]) == ["error refused kind 0"] and driver(["parse adjoint 19 1:0"]) == ["error refused kind 0"]


SHAPES = [
    ((16, 16, 4, 256, 0), (16, 16, 1, 1, 4)),
    ((64, 3, 1, 256, 0), (64, 3, 1, 1, 1)),
    ((384, 8, 2, 256, 0), (192, 1, 2, 8, 2)),
    ((320, 3, 1, 256, 0), (192, 1, 2, 3, 1)),
    ((384, 8, 2, 256, 64), (64, 4, 6, 2, 2)),
    ((300, 5, 1, 128, 0), (128, 1, 3, 5, 1)),
    ((32, 30, 3, 256, 16), (16, 16, 2, 2, 3)),
    ((32, 30, 3, 128, 16), (16, 8, 2, 4, 3)),
    ((257, 1, 1, 256, 0), (192, 1, 2, 1, 1)),
    ((1000, 2, 1, 256, 0), (256, 1, 4, 2, 1)),
    ((100, 7, 2, 64, 0), (64, 1, 2, 7, 2)),
]


def test_block_shape_of_the_row_kernels(driver):
    got = driver(["shape " + " ".join(map(str, args)) for args, _ in SHAPES])
    assert got == [" ".join(map(str, exp)) for _, exp in SHAPES]
