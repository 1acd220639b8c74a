"""Rigid bodies of IBMStepper on the HIP backend: markers moved on the device (k_ibm_move), the footprint rebuilt every step, the
force and the torque on every body (k_ibm_loads), the poses staged ahead of a native run.

The case is the small one of tests/test_gpu_ibm.py — a 24^3 periodic box, 400 markers on a sphere of radius 5.3, omega 1.2,
relaxation 0.5, 4 sweeps — with the sphere turning by 0.008 rad/step about an axis beside it and drifting, for 12 steps: marker
speeds stay <= 0.071, every marker stays in 5.99 .. 18.19 (no support is clipped), the largest displacement is 0.77 cells.

Tolerances.  rho, u and the marker forces against the restatement (tests/_ibm_ref.py fed with the positions and velocities of
tests/_ibm_motion_ref.py): 1e-6 absolute, the project's graded tolerance, as in tests/test_gpu_ibm.py.  Positions: bit for bit.
Loads: 2 n 2^-53 sum |term| per component against the sequential double sum of the same terms (derived in _ibm_motion_ref).

Measured on an MI355X: D3Q19 BGK FP32FP32 |d rho| 5.96e-7, |d u| 8.96e-8, |d F| 8.94e-8; D3Q27 KBC FP64FP32 8.99e-8 / 2.79e-8 / 2.15e-8;
the footprint of 2 069 cells differs by 148 cells at t = 11; loads within 5.7e-14 of the sequential sum (bounds from 2.4e-13)."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd import _lib
from xlb_amd.grid import grid_factory
from xlb_amd.operator.stepper import IBMBody, IBMStepper, RigidMotion

import _ibm_dynamics_ref as dref
import _ibm_motion_ref as mref
import _ibm_ref as ref
from _util import init_hip
from test_ibm_contact_on_cpu import light_sphere

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPE = (24, 24, 24)
N = 400
RADIUS = 5.3
OMEGA = 1.2
TOL = 1e-6
STEPS = 12
IBM = dict(ibm_max_iterations=4, ibm_relaxation=0.5)


def motion():
    return RigidMotion(centre=(9.0, 10.0, 11.85), axis=(0, 0, 1), rate=0.008, velocity=(0.02, 0.01, -0.005))


X0 = ref.fibonacci_sphere(N, RADIUS, (11.3, 12.6, 11.85))
AREAS = np.full(N, 4 * np.pi * RADIUS**2 / N, dtype=np.float32)
U0 = np.tile(np.array((0.02, 0.01, -0.005), dtype=np.float32), (N, 1))


def restated(n_moving=N):
    """[(X(t), U(t))] for t = 0 .. 11 with the first n_moving markers one moving body and the others as uploaded."""
    m = motion()
    return [mref.move_bodies(X0, U0, [(slice(0, n_moving), m, m.at(0)[1])], t) for t in range(STEPS)]


def case(lattice="D3Q19", policy="FP32FP32", collision="BGK"):
    init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    stepper = IBMStepper(grid=grid_factory(SHAPE), boundary_conditions=[], collision_type=collision, **IBM)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_np = orc.perturbed_init(SHAPE, lat, policy, seed=7)
    f_0.assign(f_np)
    return stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask


def calls_with_bodies(stepper, bodies, f_0, f_1, bc_mask, missing_mask, steps=STEPS):
    """Reference-style calls with the bodies declared; returns the current field, the forces and the footprints of every step."""
    markers = stepper.markers(X0, AREAS, U0)
    stepper.set_bodies(bodies)
    footprints = []
    for t in range(steps):
        f_0, f_1, forces = stepper(f_0, f_1, markers, None, None, bc_mask, missing_mask, OMEGA, t)
        f_0, f_1 = f_1, f_0
        footprints.append(np.sort(stepper.ibm_footprint()))
    return f_0, forces.numpy(), footprints, markers


@pytest.mark.parametrize("lattice,collision,policy", [("D3Q19", "BGK", "FP32FP32"), ("D3Q27", "KBC", "FP64FP32")])
def test_parity_with_the_restatement_moving_body(lattice, collision, policy):
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case(lattice, policy, collision)
    out, forces, footprints, markers = calls_with_bodies(stepper, [IBMBody(markers=slice(0, N), motion=motion())], f_0, f_1, bc_mask, missing_mask)
    o_bm, o_mm = np.zeros((1,) + SHAPE, np.uint8), np.zeros((lat.q,) + SHAPE, bool)
    exp = {"f": f_np}
    XU = restated()
    for X, U in XU:
        exp = ref.step(exp["f"], X, AREAS, U, o_bm, o_mm, [], OMEGA, lat, policy, collision, max_iterations=4, tolerance=1e-5, relaxation=0.5)
    T = orc.compute_dtype(policy)
    rho, u = orc.macroscopic(out.numpy().astype(T), lat)
    rho_e, u_e = orc.macroscopic(exp["f"].astype(T), lat)
    figures = (float(np.abs(rho.astype(np.float64) - rho_e).max()), float(np.abs(u.astype(np.float64) - u_e).max()),
               float(np.abs(forces.astype(np.float64) - exp["forces"]).max()))
    print(f"{lattice} {collision} {policy}: max |d rho| %.3e  |d u| %.3e  |d F| %.3e  (max |F| {np.abs(exp['forces']).max():.3e})" % figures)
    assert np.isfinite(out.numpy()).all()
    assert max(figures) <= TOL, figures
    assert np.abs(exp["G"]).max() > 1e-3  # (the coupling is not a no-op on these inputs)
    assert np.array_equal(markers.positions(), XU[-1][0])
    assert np.array_equal(markers.velocities(), XU[-1][1])
    # the body really moved across cells: the footprints are those of the restated positions, and the last is not the first
    assert np.array_equal(footprints[-1], np.flatnonzero(exp["W"].ravel() > 0))
    moved = np.setxor1d(footprints[0], footprints[-1]).size
    print(f"footprint {footprints[0].size} cells at t = 0, {moved} cells differ at t = {STEPS - 1}")
    assert moved > 0


def test_native_run_equals_host_driven_loop():
    results = {}
    # (a) the native run with a RigidMotion
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
    stepper.markers(X0, AREAS, U0)
    stepper.set_bodies([IBMBody(markers=slice(0, N), motion=motion())])
    cur, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, STEPS)
    results["run"] = (cur.numpy(), stepper.s_lagr_forces.numpy())
    # (b) the loop the host drives: upload the restatement's float32 positions and velocities before every call, no bodies
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
    markers = stepper.markers(X0, AREAS, U0)
    for t, (X, U) in enumerate(restated()):
        markers.update(vertices=X, velocities=U)
        f_0, f_1, forces = stepper(f_0, f_1, markers, None, None, bc_mask, missing_mask, OMEGA, t)
        f_0, f_1 = f_1, f_0
    results["host loop"] = (f_0.numpy(), forces.numpy())
    # (c) reference-style calls with the bodies declared
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
    out, forces, _, _ = calls_with_bodies(stepper, [IBMBody(markers=slice(0, N), motion=motion())], f_0, f_1, bc_mask, missing_mask)
    results["calls"] = (out.numpy(), forces)
    # (d) the native run in chunks of 5 steps (three stagings: 5 + 5 + 2)
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
    stepper.POSE_CHUNK_STEPS = 5
    stepper.markers(X0, AREAS, U0)
    stepper.set_bodies([IBMBody(markers=slice(0, N), motion=motion())])
    cur, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, STEPS)
    results["chunked run"] = (cur.numpy(), stepper.s_lagr_forces.numpy())
    assert not np.array_equal(results["run"][0], f_np)
    for name in ("host loop", "calls", "chunked run"):
        assert np.array_equal(results[name][0], results["run"][0]), name
        assert np.array_equal(results[name][1], results["run"][1]), name


def two_bodies():
    return [IBMBody(markers=slice(0, 250), motion=motion()), IBMBody(markers=slice(250, N))]


def test_body_loads():
    m = motion()
    rest_centre = X0[250:].astype(np.float64).mean(axis=0)

    def check(stepper, loads, t):
        F, X = stepper.s_lagr_forces.numpy(), stepper._markers.positions()
        assert np.array_equal(X, restated(250)[t][0])
        for b, (sl, c) in enumerate(((slice(0, 250), m.at(t)[1]), (slice(250, N), rest_centre))):
            exp, bound = mref.loads(F[sl], AREAS[sl], X[sl], c), mref.loads_bound(F[sl], AREAS[sl], X[sl], c)
            err = np.abs(loads[b] - exp)
            print(f"t = {t}, body {b}: loads {loads[b]}, max |d| {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}")
            assert (err <= bound).all(), (b, err, bound)
            assert np.abs(exp).max() > 1e-3
            assert np.array_equal(loads[b], mref.loads_tree(F[sl], AREAS[sl], X[sl], c))
        # the first column is the drag examples/sphere_ibm_hip.py prints, here split over the two bodies
        drag_terms = F[:, 0].astype(np.float64) * AREAS.astype(np.float64)
        assert abs(loads[:, 0].sum() + drag_terms.sum()) <= 2 * N * 2.0**-53 * np.abs(drag_terms).sum()

    def fresh():
        stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
        stepper.markers(X0, AREAS, U0)
        stepper.set_bodies(two_bodies())
        assert np.array_equal(stepper.body_loads(), np.zeros((2, 6)))
        return stepper, f_0, f_1, bc_mask, missing_mask

    stepper, f_0, f_1, bc_mask, missing_mask = fresh()
    _, _, one = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, 1, record_loads=True)
    assert one.shape == (1, 2, 6) and one.dtype == np.float64
    first = stepper.body_loads()
    assert np.array_equal(one[0], first)
    check(stepper, first, 0)
    histories = []
    for _ in range(2):
        stepper, f_0, f_1, bc_mask, missing_mask = fresh()
        _, _, history = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, STEPS, record_loads=True)
        histories.append(history)
    assert history.shape == (STEPS, 2, 6)
    last = stepper.body_loads()
    assert np.array_equal(history[0], first) and np.array_equal(history[-1], last)
    check(stepper, last, STEPS - 1)
    assert np.array_equal(histories[0], histories[1])
    assert not np.array_equal(history[0], history[-1])
    # without record_loads run() returns what it always did
    assert len(stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, 1, first_timestep=STEPS)) == 2


def test_resting_bodies_change_nothing():
    def run(bodies):
        stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
        stepper.markers(X0, AREAS, U0)
        for declared in bodies:
            stepper.set_bodies(declared)
        before = stepper.ibm_footprint()
        cur, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, STEPS)
        return stepper, cur.numpy(), stepper.s_lagr_forces.numpy(), before, stepper.ibm_footprint()

    _, plain_f, plain_F, _, _ = run([])
    resting = [IBMBody(markers=slice(0, 250)), IBMBody(markers=slice(300, N), centre0=(11.0, 12.0, 13.0))]
    stepper, f, F, before, after = run([resting])
    assert np.array_equal(f, plain_f) and np.array_equal(F, plain_F)
    # not rebuilt: the slots are handed out by atomics in arrival order, and the list is still the one built at the upload
    assert np.array_equal(before, after)
    assert np.array_equal(stepper._markers.positions(), X0) and np.array_equal(stepper._markers.velocities(), U0)
    loads = stepper.body_loads()
    c0 = X0[:250].astype(np.float64).mean(axis=0)
    assert (np.abs(loads[0] - mref.loads(F[:250], AREAS[:250], X0[:250], c0)) <= mref.loads_bound(F[:250], AREAS[:250], X0[:250], c0)).all()
    assert (np.abs(loads[1] - mref.loads(F[300:], AREAS[300:], X0[300:], (11.0, 12.0, 13.0)))
            <= mref.loads_bound(F[300:], AREAS[300:], X0[300:], (11.0, 12.0, 13.0))).all()
    _, f, F, _, _ = run([resting, []])
    assert np.array_equal(f, plain_f) and np.array_equal(F, plain_F)


PHASE_STEPS = 3


def run_phase(stepper, phase, f_np, f_0, f_1, bc_mask, missing_mask):
    """Three steps of one declaration from the initial populations and the uploaded markers; everything that can be read afterwards."""
    f_0.assign(f_np)
    out = {}
    if phase == "free":  # the light sphere of test_ibm_contact_on_cpu.py on a floor plane 0.25 below it (range 0.5): pushed from the first step
        floor = dref.CENTRE[2] - RADIUS - 0.25
        stepper.set_contact(0.5, 2.0, wall_stiffness=1.0, box=((-np.inf, -np.inf, floor), (np.inf,) * 3))
        stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=light_sphere(1.15, 8.0), contact_radius=RADIUS)])
        cur, _, out["poses history"] = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, PHASE_STEPS, record_poses=True)
    elif phase == "prescribed":
        stepper.set_bodies([IBMBody(markers=slice(0, N), motion=motion())])
        cur, _, out["loads history"] = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, PHASE_STEPS, record_loads=True)
    else:
        stepper.set_bodies([IBMBody(markers=slice(0, N))] if phase == "rest" else [])
        cur, _ = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, PHASE_STEPS)
    out.update({"f": cur.numpy(), "forces": stepper.s_lagr_forces.numpy(), "loads": stepper.body_loads(), "poses": stepper.body_poses(),
                "contact": stepper.body_contact_forces(), "positions": stepper._markers.positions()})
    return out


def test_redeclaring_bodies_equals_a_fresh_stepper():
    """One stepper declared four times over — a free light sphere with virtual mass on a floor, the same markers as a prescribed body,
    as a body at rest, then no bodies — against a fresh stepper for each declaration, bit for bit: a flag, a table or a recording that
    survives a redeclaration shows up here."""
    still = np.zeros_like(X0)
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
    markers = stepper.markers(X0, AREAS, still)
    got = {}
    for phase in ("free", "prescribed", "rest", "none"):
        markers.update(vertices=X0, velocities=still)
        got[phase] = run_phase(stepper, phase, f_np, f_0, f_1, bc_mask, missing_mask)
    for phase, mine in got.items():
        fresh, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
        fresh.markers(X0, AREAS, still)
        exp = run_phase(fresh, phase, f_np, f_0, f_1, bc_mask, missing_mask)
        assert mine.keys() == exp.keys()
        for what in exp:
            assert mine[what].shape == exp[what].shape and np.array_equal(mine[what], exp[what]), (phase, what)
    # every declaration did what it says
    assert (got["free"]["contact"][0, 2] > 0.0) and got["free"]["poses history"].shape == (PHASE_STEPS, 1, 18)
    assert not np.array_equal(got["free"]["positions"], X0) and not np.array_equal(got["prescribed"]["positions"], X0)
    assert got["prescribed"]["loads history"].shape == (PHASE_STEPS, 1, 6) and np.abs(got["prescribed"]["loads history"]).min(axis=2).max() > 0
    assert np.array_equal(got["prescribed"]["contact"], np.zeros((1, 3))) and np.array_equal(got["rest"]["contact"], np.zeros((1, 3)))
    assert np.array_equal(got["rest"]["positions"], X0) and np.array_equal(got["none"]["positions"], X0)
    assert np.array_equal(got["rest"]["f"], got["none"]["f"]) and not np.array_equal(got["rest"]["f"], got["prescribed"]["f"])
    assert got["none"]["loads"].shape == (0, 6) and got["none"]["poses"].shape == (0, 18)


def test_unstaged_pose_and_bad_bodies_fail_loudly():
    lib = _lib.load()
    stepper, lat, f_np, f_0, f_1, bc_mask, missing_mask = case()
    markers = stepper.markers(X0, AREAS, U0)
    native = stepper._ibm_native()
    args = (native._h, f_0.handle, f_1.handle, bc_mask.handle, missing_mask.handle, OMEGA)

    def last_error():
        return lib.xlbhip_last_error().decode()

    # bad bodies at the C entry: out of bounds, overlapping, too many
    i64 = lambda *v: np.array(v, np.int64)  # noqa: E731
    centre = np.zeros((65, 3))
    moving = np.ones(65, np.int32)
    for first, count, nb, words in ((i64(0, 300), i64(100, 101), 2, ("body 1", "out of bounds")), (i64(0, 50), i64(100, 100), 2, ("bodies 0 and 1", "overlap")),
                                    (np.arange(65, dtype=np.int64), np.ones(65, np.int64), 65, ("65 bodies", "64"))):
        assert lib.xlbhip_ibm_set_bodies(native._h, nb, first.ctypes.data, count.ctypes.data, moving.ctypes.data, centre.ctypes.data) != 0
        assert all(w in last_error() for w in words), last_error()
    with pytest.raises(ValueError, match="bodies 0 and 1 overlap"):
        stepper.set_bodies([IBMBody(slice(0, 100), motion()), IBMBody(slice(50, 150))])
    stepper.set_bodies([IBMBody(markers=slice(0, N), motion=motion())])
    with pytest.raises(_lib.HipBackendError, match="number of markers"):
        markers.update(X0[:100], AREAS[:100], U0[:100])
    # a step and a run whose poses were never staged: refused before anything is enqueued, the message names the timestep
    assert lib.xlbhip_ibm_step(*args, 7) != 0
    assert "timestep 7" in last_error() and "not staged" in last_error(), last_error()
    native.stage_poses(0, stepper._poses(0, 3))
    where = C.c_int()
    assert lib.xlbhip_ibm_run(*args, 0, 5, C.byref(where)) != 0
    assert "timestep 3" in last_error(), last_error()
    with pytest.raises(_lib.HipBackendError, match="at most"):
        native.stage_poses(0, np.zeros((8000, 1, 18)))
    assert np.array_equal(f_0.numpy(), f_np) and np.array_equal(markers.positions(), X0)  # nothing ran
    # the state is still good for a correct run
    cur, oth = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, STEPS)
    stepper2, lat, f_np, g_0, g_1, bc_mask2, missing_mask2 = case()
    stepper2.markers(X0, AREAS, U0)
    stepper2.set_bodies([IBMBody(markers=slice(0, N), motion=motion())])
    exp, _ = stepper2.run(g_0, g_1, bc_mask2, missing_mask2, OMEGA, STEPS)
    assert np.array_equal(cur.numpy(), exp.numpy())
    assert np.array_equal(markers.positions(), restated()[-1][0])
    # a later upload of the array the footprint was first built from is not mistaken for "not moved"
    markers.update(vertices=X0)
    stepper.set_bodies([])
    assert np.array_equal(markers.positions(), X0)
    stepper(cur, oth, markers, None, None, bc_mask, missing_mask, OMEGA, STEPS)
    W = ref.couple(f_np, X0, AREAS, U0, lat, "FP32FP32", relaxation=0.5)["W"]
    assert np.array_equal(np.sort(stepper.ibm_footprint()), np.flatnonzero(W.ravel() > 0))


def test_rotor_example_runs(tmp_path):
    script = os.path.join(ROOT, "examples", "rotor_ibm_hip.py")
    res = subprocess.run([sys.executable, script, "--nx", "96", "--ny", "48", "--nz", "48", "--steps", "40"], capture_output=True, text=True, timeout=300,
                         cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    for word in ("torque", "drag"):
        line = [l for l in res.stdout.splitlines() if l.startswith(word)][-1]
        assert np.isfinite(float(line.split()[-1])), line
