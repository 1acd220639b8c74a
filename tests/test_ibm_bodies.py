"""What the host decides about the rigid bodies of the immersed-boundary stepper (xlb_amd/csrc/ibm_bodies.hpp) compiled for the CPU:
the tables xlbhip_ibm_set_bodies uploads and the plan that says which launches a step makes.  Expected values, worked by hand.

Tables.  A body of `count` markers from `first` is summed in chunks of 256 consecutive markers, the last one short:

  count   chunks   (first = 7)                      chunk0
  0       0        -                                0 0
  1       1        7:1                              0 1
  255     1        7:255                            0 1
  256     1        7:256                            0 1
  257     2        7:256  263:1                     0 2
  513     3        7:256  263:256  519:1            0 3

and the six of them declared together, back to back from marker 0 (firsts 0 0 1 256 512 769, 1282 markers), have
chunk0 = 0 0 1 2 3 5 8: monotone, ending at the 8 chunks there are.  move_id is the body of a marker whose body MOVES (flag 1 or 2),
else -1.  Three bodies over 100 markers, declared in descending order with gaps — body 0 prescribed on 60:90, body 1 dynamic on
10:30, body 2 at rest on 35:50 — give move_id = 10 x -1, 20 x 1, 30 x -1 (gap 30:35, the resting body, gap 50:60), 30 x 0, 10 x -1.
The flags: any_moving = some body with flag 1 or 2 HAS markers; any_prescribed = some body with flag 1 has markers; any_dynamic =
some body has flag 2, with markers or without.  The rest pose of a body is R = identity, c = centre0, w = v = 0.

Plan.  The conditions of the launch helpers as they stood before the plan existed (csrc/ibm.hip of 4c8b425), with `recording` =
"a pose history is armed" (pose_hist_rows > 0):

  use_live   = any_dynamic or recording                       xlbhip_ibm_step: k_ibm_pose is launched iff use_live
  pose read  = live table if use_live, else the rest poses if not any_prescribed, else the timestep's staged row      ibm_pose_at
  staged     = any_prescribed                                 ibm_require_poses demands the rows; k_ibm_pose is handed the row iff so
  integrator = none if not any_dynamic; k_ibm_integrate_contact if virtual_on or contact_on, with the radii iff contact_on (else a
               null pointer); otherwise k_ibm_integrate       ibm_integrate
  move       = any_moving                                     ibm_move

tests/golden/ibm_step_plan.txt holds these for every combination of the seven flags in which virtual_on or contact_on implies
dynamics_set and dynamics_set implies any_dynamic (48 rows): `parent_plan` below restates the conditions, the file must equal it,
and the header must give the file."""

import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ibm_step_plan.txt")
FLAGS = ("any_moving", "any_prescribed", "any_dynamic", "dynamics_set", "virtual_on", "contact_on", "recording")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("ibm_bodies") / "driver"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "ibm_bodies_driver.cpp"), "-o", str(exe)], check=True, timeout=300)
    return lambda lines: subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()


def tables(n, bodies):
    """bodies: (first, count, moving[, centre0])"""
    words = [f"tables {n} {len(bodies)}"]
    for body in bodies:
        first, count, moving = body[:3]
        words.append(" ".join(map(repr, (first, count, moving) + tuple(body[3] if len(body) > 3 else (0.0, 0.0, 0.0)))))
    return " ".join(words)


def parse(lines):
    out = {}
    for line in lines:
        key, _, value = line.partition(" ")
        out[key] = value
    return out


@pytest.mark.parametrize(
    "count, chunk0, chunks, move_id, flags",
    [
        (0, "0 0", "", "-1x600", "0 0 0"),
        (1, "0 1", "0:7:1", "-1x7 0x1 -1x592", "1 1 0"),
        (255, "0 1", "0:7:255", "-1x7 0x255 -1x338", "1 1 0"),
        (256, "0 1", "0:7:256", "-1x7 0x256 -1x337", "1 1 0"),
        (257, "0 2", "0:7:256 0:263:1", "-1x7 0x257 -1x336", "1 1 0"),
        (513, "0 3", "0:7:256 0:263:256 0:519:1", "-1x7 0x513 -1x80", "1 1 0"),
    ],
)
def test_chunks_of_one_body(driver, count, chunk0, chunks, move_id, flags):
    got = parse(driver([tables(600, [(7, count, 1)])]))
    assert got == {"flags": flags, "chunk0": chunk0, "kind": "1", "chunks": chunks, "move_id": move_id, "rest": "1 0 0 0 1 0 0 0 1 0 0 0 0 0 0 0 0 0"}


def test_chunk0_is_monotone_and_ends_at_the_chunk_total(driver):
    got = parse(driver([tables(1282, [(0, 0, 1), (0, 1, 1), (1, 255, 1), (256, 256, 1), (512, 257, 1), (769, 513, 1)])]))
    assert got["chunk0"] == "0 0 1 2 3 5 8"
    assert got["chunks"] == "1:0:1 2:1:255 3:256:256 4:512:256 4:768:1 5:769:256 5:1025:256 5:1281:1"
    assert got["move_id"] == "1x1 2x255 3x256 4x257 5x513"


def test_descending_bodies_gaps_and_a_resting_body(driver):
    got = parse(driver([tables(100, [(60, 30, 1), (10, 20, 2), (35, 15, 0)])]))
    assert got["move_id"] == "-1x10 1x20 -1x30 0x30 -1x10"
    assert got["chunks"] == "0:60:30 1:10:20 2:35:15" and got["chunk0"] == "0 1 2 3"
    assert got["kind"] == "1 2 0" and got["flags"] == "1 1 1"


def test_bodies_without_markers(driver):
    # a dynamic body without markers is still integrated, but there is nothing to move; a prescribed one asks for no staged poses
    dynamic, prescribed, resting = (parse(driver([tables(10, [(0, 0, kind)])])) for kind in (2, 1, 0))
    assert dynamic["flags"] == "0 0 1" and prescribed["flags"] == "0 0 0" and resting["flags"] == "0 0 0"
    assert driver(["plan 0 0 0 0 0 0 0"]) == ["rest 0 0 none 0"]  # the plan of that prescribed body
    assert dynamic["move_id"] == prescribed["move_id"] == "-1x10" and dynamic["chunks"] == ""
    # a resting body WITH markers moves nothing either
    assert parse(driver([tables(10, [(2, 5, 0)])]))["flags"] == "0 0 0"
    # a dynamic body with markers, alone: moving, nothing prescribed
    assert parse(driver([tables(10, [(2, 5, 2)])]))["flags"] == "1 0 1"


def test_rest_poses(driver):
    got = parse(driver([tables(20, [(0, 5, 1, (1.5, -2.25, 1.0 / 3.0)), (5, 5, 0, (0.1, 1e300, -0.0))])]))
    rest = [float(v) for v in got["rest"].split()]
    eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    assert rest == eye + [1.5, -2.25, 1.0 / 3.0] + [0.0] * 6 + eye + [0.1, 1e300, -0.0] + [0.0] * 6


def test_refusals_keep_their_texts_and_their_order(driver):
    one = lambda i: (i, 1, 0)
    assert parse(driver([tables(64, [one(i) for i in range(64)])]))["chunk0"] == " ".join(map(str, range(65)))
    assert driver([tables(65, [one(i) for i in range(65)])]) == ["error 65 bodies, at most 64 are supported"]
    assert driver([tables(400, [(0, 400, 3)])]) == ["error body 0: bad moving flag 3 (0 at rest, 1 prescribed, 2 dynamic)"]
    assert driver([tables(400, [(0, 100, 2), (100, 100, -1)])]) == ["error body 1: bad moving flag -1 (0 at rest, 1 prescribed, 2 dynamic)"]
    assert driver([tables(400, [(0, 100, 0), (300, 101, 0)])]) == ["error body 1: markers 300 .. 401 are out of bounds (400 markers)"]
    assert driver([tables(400, [(-5, 100, 0)])]) == ["error body 0: markers -5 .. 95 are out of bounds (400 markers)"]
    assert driver([tables(400, [(0, 100, 0), (200, 100, 0), (99, 51, 0)])]) == ["error bodies 0 and 2 overlap"]
    assert parse(driver([tables(400, [(0, 100, 0), (100, 100, 0)])]))["chunk0"] == "0 1 2"  # touching ranges do not overlap
    # the order: the number of bodies, missing arrays, then body after body its range and its overlaps, the moving flags last
    assert driver([tables(10, [(0, 11, 3) for _ in range(65)])]) == ["error 65 bodies, at most 64 are supported"]
    assert driver(["nulls 65", "nulls 1", "nulls 0"]) == ["error 65 bodies, at most 64 are supported", "error null argument", "ok"]
    assert driver([tables(10, [(0, 11, 3)])]) == ["error body 0: markers 0 .. 11 are out of bounds (10 markers)"]
    assert driver([tables(10, [(0, 5, 3), (4, 7, 0)])]) == ["error body 1: markers 4 .. 11 are out of bounds (10 markers)"]
    assert driver([tables(10, [(0, 5, 3), (4, 2, 0)])]) == ["error bodies 0 and 1 overlap"]


def reachable():
    for flags in itertools.product((0, 1), repeat=7):
        f = dict(zip(FLAGS, flags))
        if (f["virtual_on"] or f["contact_on"]) and not f["dynamics_set"]:
            continue
        if f["dynamics_set"] and not f["any_dynamic"]:
            continue
        yield flags


def parent_plan(flags):
    """The docstring's conditions, one by one."""
    f = dict(zip(FLAGS, flags))
    use_live = bool(f["any_dynamic"] or f["recording"])
    pose = "live" if use_live else "rest" if not f["any_prescribed"] else "staged"
    if not f["any_dynamic"]:
        integrator = "none"
    elif f["virtual_on"] or f["contact_on"]:
        integrator = "contact+radius" if f["contact_on"] else "contact+null"
    else:
        integrator = "integrate"
    return f"{pose} {int(use_live)} {f['any_prescribed']} {integrator} {f['any_moving']}"


def golden_rows():
    with open(GOLDEN) as fh:
        rows = [line.split("->") for line in fh.read().splitlines() if line and not line.startswith("#")]
    return [(tuple(int(v) for v in flags.split()), plan.strip()) for flags, plan in rows]


def test_the_golden_plan_table_states_the_conditions_of_the_old_launch_helpers():
    rows = golden_rows()
    assert [flags for flags, _ in rows] == list(reachable()) and len(rows) == 48
    assert [plan for _, plan in rows] == [parent_plan(flags) for flags, _ in rows]
    table = dict(rows)
    #              moving prescribed dynamic set virtual contact recording
    assert table[(1, 0, 1, 1, 0, 0, 0)] == "live 1 0 integrate 1"  # free bodies only: the live table, no staging
    assert table[(1, 1, 0, 0, 0, 0, 0)] == "staged 0 1 none 1"  # prescribed only, nothing recorded: the staged row read directly, no k_ibm_pose
    assert table[(1, 1, 0, 0, 0, 0, 1)] == "live 1 1 none 1"  # prescribed with a pose history: the live table
    assert table[(0, 0, 0, 0, 0, 0, 0)] == "rest 0 0 none 0"  # no moving body: the rest poses
    assert table[(1, 0, 1, 1, 0, 1, 0)] == "live 1 0 contact+radius 1"  # contact without virtual mass: the contact kernel with radii
    assert table[(1, 0, 1, 1, 1, 0, 0)] == "live 1 0 contact+null 1"  # virtual mass alone: the contact kernel, null radii
    assert table[(1, 0, 1, 1, 1, 1, 0)] == "live 1 0 contact+radius 1"
    assert table[(1, 0, 1, 0, 0, 0, 0)] == "live 1 0 integrate 1"  # (dynamics not set: the step is refused before any launch)


def test_the_plan_gives_the_golden_table(driver):
    rows = golden_rows()
    got = driver(["plan " + " ".join(map(str, flags)) for flags, _ in rows])
    assert got == [plan for _, plan in rows]
