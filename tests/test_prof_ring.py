"""The bookkeeping of the ring of per-timestep profile tables (xlb_amd/csrc/prof_ring.hpp) compiled for the CPU: the slot count
of a byte budget, which slots a staging call takes and in which copy runs, which timesteps are resident afterwards.  The expected
values follow from the rules of xlbhip_stepper_stage_bc_profiles, worked by hand: 64 MiB of images, clamped to 4 .. 64 slots and
made even; slots are taken round-robin from the head, one copy per run of consecutive slots, a run ending where the ring wraps; a
taken slot loses its old timestep, and a timestep staged again lives in the newer slot only."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("prof_ring") / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "prof_ring_driver.cpp"), "-o", str(exe)], check=True, timeout=300)
    return lambda lines: subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()


def test_slot_count_of_the_byte_budget(driver):
    # 64 MiB / image, at least 4, at most 64, even: 0 B and 1 MiB -> 64; 3 MiB -> 21 -> 20; 16 MiB -> 4; 1 GiB -> 0 -> 4
    sizes = [0, MIB, 3 * MIB, 16 * MIB, 1 << 30]
    assert driver([f"slots {b}" for b in sizes]) == ["64", "64", "20", "4", "4"]
    # around the clamps: one byte over 1 MiB -> 63 -> 62; a fifth of the budget -> 5 -> 4; a sixth (rounded down) -> 6
    assert driver([f"slots {MIB + 1}", f"slots {64 * MIB // 5 + 1}", f"slots {64 * MIB // 6}"]) == ["62", "4", "6"]


def test_copy_runs_split_where_the_ring_wraps(driver):
    got = driver(["ring 4", "stage 0 3", "resident", "stage 3 3", "resident"] + [f"find {t}" for t in range(6)])
    assert got[0] == "ok"
    assert got[1] == "0,3" and got[2] == "0:0 1:1 2:2"
    assert got[3] == "3,1 0,2"  # slot 3, then the ring wraps: slots 0 and 1
    assert got[4] == "0:4 1:5 2:2 3:3"
    assert got[5:] == ["absent", "absent", "2", "3", "0", "1"]  # timesteps 2 .. 5 resident, 0 and 1 overwritten


def test_a_restaged_timestep_lives_in_the_newer_slot_only(driver):
    # timesteps 0, 1 in slots 0, 1; then 1, 2 from the head: slots 2, 3 — the older image of timestep 1 (slot 1) is superseded
    got = driver(["ring 4", "stage 0 2", "stage 1 2", "resident", "find 1", "find 0", "find 2"])
    assert got[1:3] == ["0,2", "2,2"]
    assert got[3] == "0:0 2:1 3:2"
    assert got[4:] == ["2", "0", "3"]


def test_a_whole_ring_at_once_and_nothing_at_all(driver):
    got = driver(["ring 4", "stage 7 0", "resident", "stage 0 1", "stage 1 4", "resident"])
    assert got[1] == "" and got[2] == ""  # staging nothing takes no slot
    assert got[3] == "0,1"
    assert got[4] == "1,3 0,1"  # all four slots, from the head (slot 1), split at the wrap
    assert got[5] == "0:4 1:1 2:2 3:3"


def test_a_timestep_never_staged_is_absent(driver):
    # (a fresh slot's timestep field is 0: timestep 0 must not be found in a slot that was never staged)
    got = driver(["ring 4", "find 0", "find 5", "stage 10 2", "find 0", "find 9", "find 12", "find -1", "find 10"])
    assert got == ["ok", "absent", "absent", "0,2", "absent", "absent", "absent", "absent", "0"]
