"""Virtual mass and contact forces of IBMStepper's free bodies on the HIP backend (k_ibm_integrate_contact): the device replayed bit
for bit by tests/_ibm_contact_ref.py from its own recorded loads, a coupled run of a sphere about as dense as the fluid against
the restated loop, and the launches of a stepper that uses neither feature left as they were.

The single-sphere cases are the 24^3 box and the 400-marker sphere of tests/test_gpu_ibm_dynamics.py.  Tolerances: replays are bit
for bit; rho, u and the marker forces of the coupled run are held to the project's 1e-6, c, v and w to ten times the deviation
measured on an MI355X (MEASURED_DEVIATION, profiles/ibm_virtual_mass.md) — the rule of
tests/test_gpu_ibm_dynamics.py::test_end_to_end_against_the_restatement."""

import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd import _lib
from xlb_amd.grid import grid_factory
from xlb_amd.operator.stepper import IBMBody, IBMStepper, RigidDynamics

import _ibm_contact_ref as cref
import _ibm_dynamics_ref as dref
import _ibm_ref as ref
from _util import init_hip
from test_ibm_contact_on_cpu import BAND_LIGHT_START, G10, MARGIN_LIGHT, light_sphere

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPE, N, STEPS, OMEGA = dref.SHAPE, dref.N_MARKERS, dref.COUPLED_STEPS, dref.COUPLED_OMEGA
IBM = dict(ibm_max_iterations=4, ibm_relaxation=0.5)
TOL = 1e-6
X0 = ref.fibonacci_sphere(N, dref.RADIUS, dref.CENTRE)
AREAS = np.full(N, 4 * np.pi * dref.RADIUS**2 / N, dtype=np.float32)
# max |device - restatement| over the 13 poses of the coupled run (density 1.15, C_v = 8, gravity 2^-10), measured on an MI355X:
# (c, v, w) per policy; the rotation is locked, so w is zero on both sides
MEASURED_DEVIATION = {"FP64FP64": (1.474e-13, 2.807e-14, 0.0), "FP32FP32": (1.536e-09, 4.880e-10, 0.0)}


def case(shape, X, areas, lattice="D3Q19", policy="FP32FP32", collision="BGK"):
    init_hip(lattice, policy)
    lat = orc.Lattice(lattice)
    stepper = IBMStepper(grid=grid_factory(shape), boundary_conditions=[], collision_type=collision, **IBM)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    f_np = orc.initialize_eq(shape, lat, policy)
    f_0.assign(f_np)
    stepper.markers(X, areas, np.zeros_like(X))
    return stepper, lat, f_np, (f_0, f_1, bc_mask, missing_mask)


def tables(dynamics):
    natives = [d.native() for d in dynamics]
    return (np.array([n[0] for n in natives], np.int32), np.array([n[1] for n in natives]), np.array([n[2] for n in natives]),
            np.array([d.virtual() for d in dynamics]))


@pytest.mark.parametrize("lattice,collision,policy", [("D3Q19", "BGK", "FP32FP32"), ("D3Q27", "KBC", "FP64FP32")])
def test_replay_with_virtual_mass_and_a_floor_bit_for_bit(lattice, collision, policy):
    """The light sphere, turning slowly, above a floor plane 0.25 below its lowest point (range 0.5): in contact from the first step."""
    dyn = RigidDynamics.sphere(dref.RADIUS, 1.15, dref.CENTRE, gravity=(0, 0, -G10), velocity=(0, 0, -G10 / 2), virtual_mass_coefficient=8.0,
                               angular_velocity=(2e-4, -1e-4, 3e-4))
    floor = dref.CENTRE[2] - dref.RADIUS - 0.25
    stepper, lat, f_np, fields = case(SHAPE, X0, AREAS, lattice, policy, collision)
    stepper.set_contact(0.5, 2.0, wall_stiffness=1.0, box=((-np.inf, -np.inf, floor), (np.inf,) * 3))
    stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=dyn, contact_radius=dref.RADIUS)])
    assert np.array_equal(stepper.body_contact_forces(), np.zeros((1, 3)))
    initial = stepper.body_poses()
    cur, oth, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
    rotate, P, S, virt = tables([dyn])
    assert virt.min() > 0.0
    model = cref.Contact([dref.RADIUS], 0.5, 2.0, 1.0, lo=(-np.inf, -np.inf, floor))
    exp, _, prevs, contacts = cref.replay([2], rotate, P, S, loads, virt, model)
    differ = np.argwhere(poses != exp[:STEPS])
    assert differ.size == 0, f"first differing (step, body, column): {differ[0]}, {poses[tuple(differ[0])]!r} != {exp[tuple(differ[0])]!r}"
    assert np.array_equal(initial, exp[0]) and np.array_equal(stepper.body_poses(), exp[STEPS])
    assert np.array_equal(stepper.body_contact_forces(), contacts[-1])
    # every part took part: the floor pushed at every step, the body turned and was loaded, the virtual terms were not zero
    assert (contacts[:, 0, 2] > 0.0).all() and np.array_equal(contacts[:, 0, :2], np.zeros((STEPS, 2)))
    assert np.abs(loads[:, 0, 2]).min() > 0 and np.abs(loads[:, 0, 3:]).max() > 0 and not np.array_equal(poses[0, 0, :9], poses[-1, 0, :9])
    assert np.abs(prevs[1:, 0, 2]).min() > 0 and np.abs(prevs[-1, 0, 3:]).max() > 0
    # the loads stay hydrodynamic: without the floor the same loads give another trajectory, with it they are what was recorded
    assert not np.array_equal(cref.replay([2], rotate, P, S, loads, virt, None)[0], exp)
    # a new declaration starts over: the state, a_prev and the contact force
    stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=dyn, contact_radius=dref.RADIUS)])
    assert np.array_equal(stepper.body_poses(), initial) and np.array_equal(stepper.body_contact_forces(), np.zeros((1, 3)))


# two spheres of radius 3.2 in a 24 x 24 x 32 box, 0.31 apart: the supports of their markers (two cells) stay inside the box
SHAPE2, R2, N2 = (24, 24, 32), 3.2, 150
CENTRES2 = ((12.1, 11.9, 9.5), (11.8, 12.2, 16.2))


def test_two_bodies_in_contact_replayed_bit_for_bit():
    X = np.concatenate([ref.fibonacci_sphere(N2, R2, c) for c in CENTRES2])
    areas = np.full(2 * N2, 4 * np.pi * R2**2 / N2, dtype=np.float32)
    lower = RigidDynamics.sphere(R2, 1.5, CENTRES2[0], virtual_mass_coefficient=10.0, angular_velocity=(1e-4, 2e-4, -1e-4))
    upper = RigidDynamics.sphere(R2, 1.5, CENTRES2[1], gravity=(0, 0, -G10), velocity=(0, 0, -G10 / 2), virtual_mass_coefficient=10.0,
                                 angular_velocity=(0.0, 0.0, 3e-4), rotate=("axis", (0.0, 0.0, 1.0)))
    stepper, lat, f_np, fields = case(SHAPE2, X, areas)
    stepper.set_bodies([IBMBody(markers=slice(0, N2), dynamics=lower, contact_radius=R2), IBMBody(markers=slice(N2, 2 * N2), dynamics=upper, contact_radius=R2)])
    stepper.set_contact(0.5, 0.5)  # (after set_bodies: it applies to the bodies declared)
    cur, oth, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
    rotate, P, S, virt = tables([lower, upper])
    assert list(rotate) == [dref.FREE, dref.AXIS]
    exp, _, prevs, contacts = cref.replay([2, 2], rotate, P, S, loads, virt, cref.Contact([R2, R2], 0.5, 0.5))
    differ = np.argwhere(poses != exp[:STEPS])
    assert differ.size == 0, f"first differing (step, body, column): {differ[0]}, {poses[tuple(differ[0])]!r} != {exp[tuple(differ[0])]!r}"
    assert np.array_equal(stepper.body_poses(), exp[STEPS])
    got = stepper.body_contact_forces()
    assert np.array_equal(got, contacts[-1]) and np.array_equal(got[0], -got[1]) and got[1, 2] > 0.0 and np.abs(got).min() > 0.0
    assert np.array_equal(contacts[:, 0], -contacts[:, 1])
    assert np.abs(loads[:, :, :3]).max(axis=(0, 2)).min() > 0 and np.isfinite(cur.numpy()).all()
    assert poses[-1, 0, 11] < CENTRES2[0][2] and not np.array_equal(poses[-1, 1, :9], poses[0, 1, :9])  # the lower one was pushed down; the upper turned


@functools.lru_cache(maxsize=None)
def restated(policy):
    lat = orc.Lattice("D3Q19")
    return cref.coupled_run(light_sphere(1.15, 8.0), X0, AREAS, orc.initialize_eq(SHAPE, lat, policy), lat, policy, "BGK", STEPS, OMEGA, dref.COUPLED_IBM)


@pytest.mark.parametrize("policy", ["FP64FP64", "FP32FP32"])
def test_light_sphere_end_to_end_against_the_restatement(policy):
    """Density 1.15, C_v = 8, gravity 2^-10 (all four sweeps run), rotation locked, 12 steps: the whole loop on the device against
    the same loop in NumPy.  Measured on an MI355X, max |device - restatement| (max |F| 5.8e-4, |u| 3.1e-4, |v| 4.9e-4, |load| 0.69):
    FP64FP64  |d rho| 4.64e-13  |d u| 1.09e-12  |d F| 4.38e-13   |d c| 1.47e-13  |d v| 2.81e-14  |d w| 0   |d loads| 8.7e-11
    FP32FP32  |d rho| 4.77e-07  |d u| 9.87e-08  |d F| 9.19e-08   |d c| 1.54e-09  |d v| 4.88e-10  |d w| 0   |d loads| 7.6e-06
    The bounds on c, v, w are ten times these (MEASURED_DEVIATION).  Unlike the heavy sphere at gravity 2^-20, the scales here are
    hundreds of times the 1e-6 bound on rho, u and F: a coupling that did nothing would miss it by far."""
    stepper, lat, f_np, fields = case(SHAPE, X0, AREAS, "D3Q19", policy, "BGK")
    dyn = light_sphere(1.15, 8.0)
    stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=dyn)])
    cur, _, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
    assert stepper.ibm_iterations_used == 4
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
    print(f"{policy}: max |d c| %.3e  |d v| %.3e  |d w| %.3e  (|v| {np.abs(exp['poses'][:, 15:18]).max():.3e})" % dev)
    print(f"{policy}: max |d loads| {np.abs(loads[:, 0] - exp['loads']).max():.3e} (max |load| {np.abs(exp['loads']).max():.3e})")
    vz = poses[:, 17] / G10
    print(f"{policy}: v_z / g", vz.round(4))
    assert np.isfinite(cur.numpy()).all()
    assert max(figures) <= TOL, figures
    assert np.abs(exp["forces"]).max() > 100 * TOL  # (the coupling is far from a no-op on these inputs)
    assert vz[1:].min() >= BAND_LIGHT_START[0] - MARGIN_LIGHT and vz[1:].max() <= BAND_LIGHT_START[1] + MARGIN_LIGHT
    for got, measured in zip(dev, MEASURED_DEVIATION[policy]):
        assert got <= 10.0 * measured, (dev, MEASURED_DEVIATION[policy])


def test_unused_features_leave_the_run_as_it_was():
    """virtual_mass = 0 and a contact model no body takes part in: populations, marker forces, loads and poses of the plain run, and
    the launches too (the native object keeps both switched off)."""
    def run(unused):
        kw = dict(virtual_mass=0.0, virtual_inertia=0.0) if unused else {}
        dyn = RigidDynamics.sphere(dref.RADIUS, dref.DENSITY, dref.CENTRE, gravity=(0, 0, -dref.GRAVITY), velocity=(0, 0, -dref.GRAVITY / 2),
                                   angular_velocity=(2e-7, -1e-7, 3e-7), **kw)
        stepper, lat, f_np, fields = case(SHAPE, X0, AREAS)
        if unused:
            stepper.set_contact(0.5, 1.0, box=((2.0, 2.0, 6.4), (22.0, 22.0, 22.0)))
        with pytest.warns(RuntimeWarning, match="body 0: mass 935"):  # (as tests/test_gpu_ibm_dynamics.py: the two-sweep regime)
            stepper.set_bodies([IBMBody(markers=slice(0, N), dynamics=dyn)])
        cur, _, loads, poses = stepper.run(*fields, OMEGA, STEPS, record_loads=True, record_poses=True)
        return stepper, (cur.numpy(), stepper.s_lagr_forces.numpy(), loads, poses, stepper.body_poses())

    stepper, a = run(True)
    _, b = run(False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[3][0], a[3][-1]) and np.array_equal(stepper.body_contact_forces(), np.zeros((1, 3)))
    # the native entry points name what they refuse
    native, two = stepper._ibm_native(), np.zeros(2)
    for call, word in ((lambda: native.set_virtual_mass([-1.0], [0.0]), "virtual_mass"), (lambda: native.set_virtual_mass([0.0], [np.inf]), "virtual_inertia"),
                       (lambda: _lib.check(_lib.load().xlbhip_ibm_set_virtual_mass(native._h, 2, two.ctypes.data, two.ctypes.data)), "2 bodies, 1 are declared"), (lambda: native.set_contact([-2.0], 0.5, 1.0, 1.0), "radius"),
                       (lambda: native.set_contact([2.0], np.nan, 1.0, 1.0), "range"), (lambda: native.set_contact([2.0], 0.5, 1.0, -1.0), "wall_stiffness"),
                       (lambda: native.set_contact([2.0], 0.5, 1.0, 1.0, (0.0, 0.0, 5.0), (9.0, 9.0, 5.0)), r"lo\[2\]")):
        with pytest.raises((_lib.HipBackendError, ValueError), match=word):
            call()


def test_light_sphere_lands_on_the_floor_in_the_example(tmp_path):
    """The example at its smallest size: density 1.15 with C_v = 8 released 1.1 cells above the floor plane, 0.1 outside the contact
    range.  It settles at 2.2e-4 cells per step (measured on an MI355X) and is overdamped on the plane: the approach to the resting
    gap 1 - sqrt(weight / stiffness) = 0.76 decays with a time constant of about 550 steps (stiffness 2 k_w p = 0.48 against the
    drag weight / speed = 266), so 10 000 steps leave it at rest.  "At rest": within the range of the plane, slower than 2 % of its
    settling speed, and carried by the contact force to 5 % of its weight.  No state was refused (the example raises on a status
    bit)."""
    script = os.path.join(ROOT, "examples", "settling_sphere_ibm_hip.py")
    args = ["--size", "24", "--density", "1.15", "--virtual-mass", "8", "--floor", "--drop", "1.1", "--gravity", "2e-3", "--steps", "10000", "--every", "500"]
    res = subprocess.run([sys.executable, script] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    print(res.stdout)
    rows = [line.split() for line in res.stdout.splitlines() if line.startswith("step")]
    cz, vz = np.array([float(r[3]) for r in rows]), np.array([float(r[5]) for r in rows])
    gap, lift, weight = (float(x) for x in re.search(r"gap above the floor plane (\S+) .* contact force (\S+) against the weight (\S+),", res.stdout).groups())
    assert len(rows) == 21 and np.isfinite(cz).all() and np.isfinite(vz).all()
    assert 0.0 < gap < 1.0 and cz[-1] < cz[0] - 0.1  # it fell and sits within the range (1 cell) of the plane
    fastest = np.abs(vz).max()
    assert fastest > 1e-4 and np.abs(vz[-5:]).max() < min(0.02 * fastest, np.abs(vz[1:4]).min())  # at rest, |v| has fallen
    assert abs(lift - weight) < 0.05 * weight  # the plane carries the weight
