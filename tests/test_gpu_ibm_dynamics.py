"""Free rigid bodies of IBMStepper on the HIP backend: the pose table written on the device (k_ibm_pose), the integrator that
advances a body from the loads of every step (k_ibm_integrate), a whole run enqueued without a host wait.

The case is the one tests/_ibm_dynamics_ref.py states and pins on the CPU: the sphere of tests/test_gpu_ibm_motion.py (24^3 periodic
box, 400 markers, radius 5.3, omega 1.2, relaxation 0.5, 4 sweeps) as a free body of density 2.5 released under gravity 2^-20 along
-z in a fluid at rest, 12 steps.

Tolerances.  The integrator against the restatement fed with the device's own loads: bit for bit (this is also the check that fp64
division and square root in device code give the host's correctly rounded bits).  rho, u and the marker forces of the whole coupled
run against the restatement: 1e-6 absolute, the project's graded tolerance.  c, v, w of that run: ten times the deviation measured
on an MI355X (the chain loads -> velocity -> float32 marker rounding -> footprint is not derivable more tightly):
MEASURED_DEVIATION below."""

import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.grid import grid_factory
from xlb_amd.operator.stepper import IBMBody, IBMStepper, RigidDynamics, RigidMotion

import _ibm_dynamics_ref as dref
import _ibm_motion_ref as mref
import _ibm_ref as ref
from _util import init_hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPE, N, STEPS, OMEGA = dref.SHAPE, dref.N_MARKERS, dref.COUPLED_STEPS, dref.COUPLED_OMEGA
IBM = dict(ibm_max_iterations=4, ibm_relaxation=0.5)
TOL = 1e-6
X0 = ref.fibonacci_sphere(N, dref.RADIUS, dref.CENTRE)
AREAS = np.full(N, 4 * np.pi * dref.RADIUS**2 / N, dtype=np.float32)
ZEROS = np.zeros((N, 3), np.float32)
# max |device - restatement| over the 13 poses of the coupled run, measured on an MI355X: (c, v, w) per policy
MEASURED_DEVIATION = {"FP64FP64": (5.151e-14, 9.133e-15, 3.898e-15), "FP32FP32": (2.116e-10, 1.719e-10, 1.584e-11)}


def sphere(**kw):
    return RigidDynamics.sphere(dref.RADIUS, dref.DENSITY, dref.CENTRE, gravity=(0, 0, -dref.GRAVITY), velocity=(0, 0, -dref.GRAVITY / 2), **kw)


def case(lattice="D3Q19", policy="FP32FP32", collision="BGK", perturbed=False):
    init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    stepper = IBMStepper(grid=grid_factory(SHAPE), boundary_conditions=[], collision_type=collision, **IBM)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_np = orc.perturbed_init(SHAPE, lat, policy, seed=7) if perturbed else orc.initialize_eq(SHAPE, lat, policy)
    f_0.assign(f_np)
    stepper.markers(X0, AREAS, ZEROS)
    return stepper, lat, f_np, (f_0, f_1, bc_mask, missing_mask)


class Recorded:
    """Recorded poses (n, 18) as a motion."""

    def __init__(self, rows):
        self.rows = rows

    def at(self, t):
        row = self.rows[int(t)]
        return row[0:9].reshape(3, 3), row[9:12], row[12:15], row[15:18]


@pytest.mark.parametrize("lattice,collision,policy", [("D3Q19", "BGK", "FP32FP32"), ("D3Q27", "KBC", "FP64FP32")])
def test_integrator_replay_bit_for_bit_and_the_staged_path(lattice, collision, policy):
    # (1) one free body, turning slowly as well; the recorded loads fed to the restatement give the recorded poses
    dyn = sphere(angular_velocity=(2e-7, -1e-7, 3e-7))
    stepper, lat, f_np, fields = case(lattice, policy, collision)
    stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=dyn)])
    initial = stepper.body_poses()
    cur, oth, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
    assert loads.shape == (STEPS, 1, 6) and poses.shape == (STEPS, 1, 18) and poses.dtype == np.float64
    rotate, P, S = dyn.native()
    exp, _ = dref.replay(rotate, P, S, loads[:, 0])
    differ = np.argwhere(poses[:, 0] != exp[:STEPS])
    assert differ.size == 0, f"first differing (step, column): {differ[0]}, {poses[tuple(differ[0])]!r} != {exp[tuple(differ[0])]!r}"
    assert np.array_equal(initial[0], exp[0])
    assert np.array_equal(stepper.body_poses()[0], exp[STEPS])
    assert np.abs(loads[:, 0, 2]).min() > 0 and np.abs(loads[:, 0, 3:]).max() > 0 and not np.array_equal(poses[0, 0, :9], poses[-1, 0, :9])
    free_f, free_F = cur.numpy(), stepper.s_lagr_forces.numpy()
    assert len(stepper.run(cur, oth, fields[2], fields[3], OMEGA, 1, first_timestep=STEPS)) == 2  # as before without record_poses
    # a new set_bodies resets the state to the declared initial values
    stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=dyn)])
    assert np.array_equal(stepper.body_poses(), initial)
    # (2) the same markers as a PRESCRIBED body following the recorded poses: the staged path gives the same bits
    stepper, lat, f_np, fields = case(lattice, policy, collision)
    stepper.set_bodies([IBMBody(markers=slice(0, N), motion=Recorded(np.concatenate([poses[:, 0], exp[STEPS:]])), centre0=dyn.centre)])
    cur, _, loads2 = stepper.run(*fields, OMEGA, STEPS, record_loads=True)
    assert np.array_equal(cur.numpy(), free_f) and np.array_equal(stepper.s_lagr_forces.numpy(), free_F)
    assert np.array_equal(loads2, loads)
    assert np.array_equal(stepper.body_poses()[0], exp[STEPS])


def heavy():
    return RigidDynamics(mass=3.0e4, inertia=1.0e6, centre=dref.CENTRE, force=(0.0, 0.0, -3.0e4 * 2.0**-12), angular_velocity=(0.0, 1e-4, 0.0))


def prescribed():
    return RigidMotion(centre=dref.CENTRE, axis=(0, 0, 1), rate=0.002, velocity=(0.001, 0.0005, 0.0))


def test_native_run_equals_reference_style_calls():
    """A free body (markers 0 .. 250) next to a prescribed one (250 .. 400): the native run, reference-style calls and a run staged
    in chunks of 5 steps give the same bits; a run with the free body alone is ONE native call and stages nothing."""
    bodies = lambda: [IBMBody(markers=slice(0, 250), dynamics=heavy()), IBMBody(markers=slice(250, N), motion=prescribed())]  # noqa: E731
    results = {}
    for name in ("run", "chunked run"):
        stepper, lat, f_np, fields = case()
        if name == "chunked run":
            stepper.POSE_CHUNK_STEPS = 5
        stepper.set_bodies(bodies())
        cur, _, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
        results[name] = (cur.numpy(), stepper.s_lagr_forces.numpy(), loads, poses, stepper.body_poses())
    stepper, lat, f_np, (f_0, f_1, bc_mask, missing_mask) = case()
    stepper.set_bodies(bodies())
    loads, poses = [], []
    for t in range(STEPS):
        poses.append(stepper.body_poses())
        f_0, f_1, forces = stepper(f_0, f_1, stepper._markers, None, None, bc_mask, missing_mask, OMEGA, t)
        f_0, f_1 = f_1, f_0
        loads.append(stepper.body_loads())
    results["calls"] = (f_0.numpy(), forces.numpy(), np.array(loads), np.array(poses), stepper.body_poses())
    assert not np.array_equal(results["run"][0], f_np)
    for name in ("chunked run", "calls"):
        for a, b in zip(results[name], results["run"]):
            assert np.array_equal(a, b), name
    poses = results["run"][3]
    m = prescribed()
    for t in (0, 7, STEPS - 1):  # the prescribed body appears with its staged rows
        R, c, w, v = m.at(t)
        assert np.array_equal(poses[t, 1], np.concatenate([np.asarray(R).reshape(9), c, w, v]))
    R, c, w, v = m.at(STEPS)
    assert np.array_equal(results["run"][4][1], np.concatenate([np.asarray(R).reshape(9), c, w, v]))
    stepper.set_bodies(bodies())  # a new declaration starts over for both kinds
    assert np.array_equal(stepper.body_poses(), poses[0])
    assert poses[-1, 0, 11] < poses[0, 0, 11] and not np.array_equal(poses[-1, 0, :9], poses[0, 0, :9])  # the free body fell and turned
    # the free body alone: one native call for all steps, no staging
    stepper, lat, f_np, fields = case()
    stepper.set_bodies([IBMBody(markers=slice(0, 250), dynamics=heavy())])
    native, count = stepper._ibm_native(), {"run": 0, "stage_poses": 0, "step": 0}
    for method in count:
        def counted(*a, _orig=getattr(native, method), _name=method):
            count[_name] += 1
            return _orig(*a)
        setattr(native, method, counted)
    stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
    assert count == {"run": 1, "stage_poses": 0, "step": 0}


def test_axis_mode_on_a_spring_and_new_reference_vertices():
    """The parts of the integrator the falling sphere does not reach, on the device: a rotor free to spin about z on a damped spring
    along z only — replayed bit for bit from its recorded loads — and ``markers.update(vertices=...)`` under a free body: the new
    vertices are the new X0, placed by the pose the state has reached."""
    anchor = (dref.CENTRE[0], dref.CENTRE[1], dref.CENTRE[2] + 0.25)
    dyn = RigidDynamics(mass=2.0e4, inertia=np.diag([8.0e5, 9.0e5, 1.0e6]), centre=dref.CENTRE, angular_velocity=(0.0, 0.0, 1e-3), torque=(0.0, 0.0, 100.0),
                        spring=(anchor, (0.0, 0.0, 50.0), 2.0), translate=(False, False, True), rotate=("axis", (0.0, 0.0, 2.0)))
    stepper, lat, f_np, fields = case(perturbed=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # a body this heavy is declared without a warning
        stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=dyn)])
    cur, oth, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
    rotate, P, S = dyn.native()
    assert rotate == dref.AXIS
    exp, states = dref.replay(rotate, P, S, loads[:, 0])
    assert np.array_equal(poses[:, 0], exp[:STEPS]) and np.array_equal(stepper.body_poses()[0], exp[STEPS])
    assert np.array_equal(exp[:, 9:11], np.tile(dref.CENTRE[:2], (STEPS + 1, 1)))  # x and y are masked
    assert exp[-1, 11] > dref.CENTRE[2] + 1e-3 and abs(states[-1, 10] - 1e-3) > 1e-5 and np.abs(loads[:, 0, 5]).max() > 1e-4  # pulled up, rate changed, loaded
    # new reference vertices (a smaller sphere): the state goes on, the markers are placed from the new X0
    X1 = (np.asarray(dref.CENTRE) + 0.9 * (X0.astype(np.float64) - dref.CENTRE)).astype(np.float32)
    stepper._markers.update(vertices=X1)
    _, _, one = stepper.run(cur, oth, fields[2], fields[3], OMEGA, 1, first_timestep=STEPS, record_poses=True)
    assert np.array_equal(one[0, 0], exp[STEPS])
    row = one[0, 0]
    X, V = mref.move(X1, dyn.centre, row[:9].reshape(3, 3), row[9:12], row[12:15], row[15:18])
    assert np.array_equal(stepper._markers.positions(), X) and np.array_equal(stepper._markers.velocities(), V)
    assert not np.array_equal(X, X1)


def test_all_locked_equals_at_rest():
    def run(body):
        stepper, lat, f_np, fields = case(perturbed=True)
        stepper.set_bodies([body])
        cur, _, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
        return cur.numpy(), stepper.s_lagr_forces.numpy(), loads, poses, stepper._markers.positions(), stepper._markers.velocities()

    locked = RigidDynamics(mass=100.0, inertia=1000.0, centre=dref.CENTRE, translate=(False,) * 3, rotate="locked")
    a = run(IBMBody(markers=slice(0, N), dynamics=locked))
    b = run(IBMBody(markers=slice(0, N), motion=None, centre0=dref.CENTRE))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    rest = np.concatenate([np.eye(3).reshape(9), dref.CENTRE, np.zeros(6)])
    assert np.array_equal(a[3], np.tile(rest, (STEPS, 1, 1)))  # a body at rest appears with its rest pose
    assert np.abs(a[2]).max() > 1e-3 and np.array_equal(a[4], X0)


def test_a_state_that_is_not_finite_is_reported():
    stepper, lat, f_np, fields = case()
    runaway = RigidDynamics(mass=1e-300, inertia=1.0, centre=dref.CENTRE, force=(1e300, 0.0, 0.0), rotate="locked")
    stepper.set_bodies([IBMBody(markers=slice(0, 100)), IBMBody(markers=slice(100, N), dynamics=runaway)])
    before = stepper.body_poses()
    cur, _ = stepper.run(*fields, OMEGA, 2)
    with pytest.raises(RuntimeError, match=r"bodies \[1\]"):
        stepper.body_poses()
    assert np.array_equal(stepper._markers.positions(), X0) and np.isfinite(cur.numpy()).all()  # the body stood still
    stepper.set_bodies([IBMBody(markers=slice(0, 100)), IBMBody(markers=slice(100, N), dynamics=runaway)])
    assert np.array_equal(stepper.body_poses(), before)  # a new declaration clears the status word


@functools.lru_cache(maxsize=None)
def restated(policy):
    lat = orc.Lattice("D3Q19")
    return dref.coupled_run(sphere(), X0, AREAS, orc.initialize_eq(SHAPE, lat, policy), lat, policy, "BGK")


@pytest.mark.parametrize("policy", ["FP64FP64", "FP32FP32"])
def test_end_to_end_against_the_restatement(policy):
    """Measured on an MI355X, max |device - restatement| (D3Q19 BGK, 12 steps; max |F| 2.7e-6, |u| 1.1e-6, |v| 2.3e-6, |load| 8.8e-4):
    FP64FP64  |d rho| 4.39e-13  |d u| 1.15e-12  |d F| 5.61e-13   |d c| 5.15e-14  |d v| 9.13e-15  |d w| 3.90e-15   |d loads| 5.4e-11
    FP32FP32  |d rho| 4.77e-07  |d u| 4.47e-08  |d F| 1.44e-08   |d c| 2.12e-10  |d v| 1.72e-10  |d w| 1.58e-11   |d loads| 3.3e-07
    The bounds on c, v, w are ten times these (MEASURED_DEVIATION); |d c| at FP64FP64 is seven orders below 1e-6.

    What discriminates.  At this gravity max |u| is 1.1e-6 and max |F| 2.7e-6, so the project's 1e-6 absolute bound on rho, u and F
    alone would nearly pass a coupling that did nothing.  The checks that bite are the bounds on c, v, w, the bit-for-bit replay and
    staged-path tests above, and the RELATIVE bounds asserted here: |d u| <= 0.25 max |u| and |d F| <= 0.25 max |F|.  Their size is
    reasoned, not measured: a coupling that did nothing misses by 100 %; fp32 rounding cannot reach 25 % — u is a sum of ten
    populations of at most 1/3, each addition rounding a partial sum below 1/2 by at most 2^-25 = 3e-8, so at worst 1.5e-7 (14 % of
    max |u|), and F adds two interpolated (averaged) deficits, at worst 3e-7 (11 % of max |F|)."""
    stepper, lat, f_np, fields = case("D3Q19", policy, "BGK")
    dyn = sphere()
    # mass 935 against 4 sweeps x 353 of marker area: declared with a warning (the run stays in the two-sweep regime, see dref)
    with pytest.warns(RuntimeWarning, match="body 0: mass 935.* is below ibm_max_iterations x sum of marker areas = 1412"):
        stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=dyn)])
    cur, _, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
    poses = np.concatenate([poses[:, 0], stepper.body_poses()])
    exp = restated(policy)
    T = orc.compute_dtype(policy)
    rho, u = orc.macroscopic(cur.numpy().astype(T), lat)
    rho_e, u_e = orc.macroscopic(exp["f"].astype(T), lat)
    forces = stepper.s_lagr_forces.numpy()
    figures = (float(np.abs(rho.astype(np.float64) - rho_e).max()), float(np.abs(u.astype(np.float64) - u_e).max()),
               float(np.abs(forces.astype(np.float64) - exp["forces"]).max()))
    print(f"{policy}: max |d rho| %.3e  |d u| %.3e  |d F| %.3e  (max |F| {np.abs(exp['forces']).max():.3e}, max |u| {np.abs(u_e).max():.3e})" % figures)
    dev = tuple(float(np.abs(poses[:, a:b] - exp["poses"][:, a:b]).max()) for a, b in ((9, 12), (15, 18), (12, 15)))
    print(f"{policy}: max |d c| %.3e  |d v| %.3e  |d w| %.3e  (|v| {np.abs(exp['poses'][:, 15:18]).max():.3e}, |w| {np.abs(exp['poses'][:, 12:15]).max():.3e})" % dev)
    print(f"{policy}: max |d loads| {np.abs(loads[:, 0] - exp['loads']).max():.3e} (max |load| {np.abs(exp['loads']).max():.3e})")
    assert np.isfinite(cur.numpy()).all()
    assert max(figures) <= TOL, figures
    assert np.abs(exp["forces"]).max() > 1e-6  # (the coupling is not a no-op on these inputs)
    assert figures[1] <= 0.25 * np.abs(u_e).max() and figures[2] <= 0.25 * np.abs(exp["forces"]).max(), figures
    dref.check_fall(poses, dyn)  # the device's own trajectory: the reaction opposes the fall and does not reverse it
    for got, measured in zip(dev, MEASURED_DEVIATION[policy]):
        assert got <= 10.0 * measured, (dev, MEASURED_DEVIATION[policy])


def test_settling_sphere_example_runs(tmp_path):
    script = os.path.join(ROOT, "examples", "settling_sphere_ibm_hip.py")
    res = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    rows = [line.split() for line in res.stdout.splitlines() if line.startswith("step")]
    cz = np.array([float(r[3]) for r in rows])
    assert len(cz) >= 5 and np.isfinite(cz).all() and (np.diff(cz) < 0).all(), res.stdout[-2000:]
