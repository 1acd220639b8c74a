"""The launch plan of the two-step kernel (xlb_amd/csrc/step2_plan.hpp) compiled for the CPU: for a table of steppers and boxes
its eligibility, the fuse decision of fuse2 = 1 / 2, the tile, the x segments, and the hull-first tile order.  The expected values
(tests/golden/step2_plan.txt) were recorded from the rules as api.hip and step2_d3q19.hip stated them before they moved into the
header: the move must not change a single launch decision."""

import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "step2_plan.txt")

D3Q19, D3Q27 = 1, 2
BGK, KBC = 0, 1
EQUILIBRIUM, HALFWAY_BB, FULLWAY_BB = 1, 2, 3
SHAPES = [((n, n, n), 0) for n in (128, 256, 320, 384, 512)] + [((4096, 512, 512), 2)]  # (shape, ghost planes per side)
# has_bc, n_bc, kinds_packed (lid, walls), needs_missing
BCS = {"periodic": (0, 0, 0, 0), "cavity_halfway": (1, 2, EQUILIBRIUM | HALFWAY_BB << 4, 1), "cavity_fullway": (1, 2, EQUILIBRIUM | FULLWAY_BB << 4, 0)}
ORDERS = [(1, 1), (1, 8), (2, 2), (3, 4), (4, 3), (8, 1), (8, 8), (9, 10)]


def cases():
    for (shape, halo), bc, lattice, collision, fuse2, cus in itertools.product(SHAPES, BCS, (D3Q19, D3Q27), (BGK, KBC), (1, 2), (256, 2)):
        yield "case " + " ".join(map(str, (*shape, halo, *BCS[bc], lattice, collision, fuse2, cus)))


def checksum(order):
    return sum((i + 1) * v for i, v in enumerate(order)) % (1 << 32)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("step2_plan") / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(ROOT, 'include')}", f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "step2_plan_driver.cpp"), "-o", str(exe)], check=True, timeout=300)
    return lambda lines: subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()


@pytest.fixture(scope="module")
def expected():
    table = {}
    for line in open(GOLDEN):
        if line.strip() and not line.startswith("#"):
            query, answer = line.split("|")
            table[query.strip()] = answer.strip()
    return table


def test_decisions_match_the_recorded_table(driver, expected):
    queries = list(cases())
    assert len(queries) == 288 and set(queries) == {q for q in expected if q.startswith("case ")}
    got = driver(queries)
    assert len(got) == len(queries)
    wrong = [f"{q} -> {g} (expected {expected[q]})" for q, g in zip(queries, got) if g != expected[q]]
    assert not wrong, "\n".join(wrong[:20])
    # the headline workload: the 512^3 halfway cavity fuses on (8 x 64) tiles in 8 x-segments
    assert expected["case 512 512 512 0 1 2 33 1 1 0 1 256"] == "1 1 8 64 8"


def test_tile_order_matches_the_recorded_table(driver, expected):
    queries = [f"order {tys} {tzs}" for tys, tzs in ORDERS]
    for q, g in zip(queries, driver(queries)):
        assert g == expected[q], q
    (big,) = driver(["order 64 8"])
    order = [int(v) for v in big.split()]
    assert sorted(order) == list(range(64 * 8))
    assert f"checksum {checksum(order)}" == expected["order 64 8"]
