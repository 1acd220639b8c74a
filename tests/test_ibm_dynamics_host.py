"""The free-body integrator of IBMStepper without a GPU: tests/_ibm_dynamics_ref.py — the restatement the kernel follows — pinned
from theory (closed forms with dyadic values, conservation laws, derived rounding bounds), the argument checks of RigidDynamics and
IBMBody, and the sanity pin of the coupled case that tests/test_gpu_ibm_dynamics.py reuses."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.helper.ibm_helper import IBMBody, RigidDynamics, RigidMotion
from xlb_amd.operator.stepper import RigidDynamics as exported_dynamics

import _ibm_dynamics_ref as dref
import _ibm_ref as ref

ZERO = np.zeros(6)


def run(dyn, loads):
    rotate, P, S = dyn.native()
    return dref.replay(rotate, P, S, loads)


def test_names_are_exported():
    from xlb_amd import helper

    assert exported_dynamics is RigidDynamics and helper.RigidDynamics is RigidDynamics


def test_translation_closed_form_with_dyadic_values():
    """Zero hydrodynamic loads, a constant force: c_n = c0 + n v0 + (force / mass) n (n + 1) / 2 and v_n = v0 + n force / mass — exact,
    every value being a dyadic rational of few bits."""
    n = 40
    c0, v0, force, mass = np.array([9.5, 10.25, 11.75]), np.array([0.125, -0.0625, 0.03125]), np.array([0.5, -0.25, 1.0]), 64.0
    dyn = RigidDynamics(mass=mass, inertia=100.0, centre=c0, velocity=v0, force=force, rotate="locked")
    poses, states = run(dyn, np.zeros((n, 6)))
    k = np.arange(n + 1)[:, None]
    assert np.array_equal(states[:, 0:3], c0 + k * v0 + (force / mass) * (k * (k + 1) / 2))
    assert np.array_equal(states[:, 3:6], v0 + k * (force / mass))
    assert np.array_equal(poses[:, 9:12], states[:, 0:3]) and np.array_equal(poses[:, 15:18], states[:, 3:6])
    assert np.array_equal(poses[:, 0:9], np.tile(np.eye(3).reshape(9), (n + 1, 1))) and not poses[:, 12:15].any()  # locked
    # masked axes do not move, whatever pushes them; the free axis is as before
    masked = RigidDynamics(mass=mass, inertia=100.0, centre=c0, velocity=(0.0, 0.0, v0[2]), force=force, translate=(False, False, True), rotate="locked")
    loads = np.random.default_rng(2).normal(size=(n, 6))
    loads[:, 2] = 0.0
    _, s2 = run(masked, loads)
    assert np.array_equal(s2[:, 0:2], np.tile(c0[0:2], (n + 1, 1))) and not s2[:, 3:5].any()
    assert np.array_equal(s2[:, 2], states[:, 2]) and np.array_equal(s2[:, 5], states[:, 5])


def test_spring_is_the_symplectic_euler_recurrence():
    n = 50
    anchor, k, mass = np.array([10.0, 11.0, 12.0]), np.array([0.3, 0.0, 1.7]), 37.0
    c, v = np.array([10.4, 11.0, 11.1]), np.array([0.0, 0.02, -0.01])
    dyn = RigidDynamics(mass=mass, inertia=1.0, centre=c, velocity=v, spring=(anchor, k, 0.0), force=(0.0, 0.0, 0.05), rotate="locked")
    _, states = run(dyn, np.zeros((n, 6)))
    inv = 1.0 / mass
    force = np.array([0.0, 0.0, 0.05])
    for t in range(n):
        assert np.array_equal(states[t, 0:3], c) and np.array_equal(states[t, 3:6], v)
        v = v + ((force - k * (c - anchor)) - 0.0 * v) * inv  # the velocity first, with the OLD position ...
        c = c + v  # ... then the position with the NEW velocity
    # the scheme is symplectic: the oscillation neither grows nor decays (x axis: amplitude 0.4 about the anchor)
    x = states[:, 0] - anchor[0]
    assert 0.39 < np.abs(x).max() <= 0.4 * (1 + 0.3 / mass)
    # a scalar stiffness and damping are broadcast
    d2 = RigidDynamics(mass=1.0, inertia=1.0, centre=c, spring=(anchor, 0.5, 0.25))
    assert np.array_equal(d2.stiffness, np.full(3, 0.5)) and np.array_equal(d2.damping, np.full(3, 0.25))


def tilted():
    return RigidMotion((0, 0, 0), (1.0, 2.0, -0.5), 0.7).at(1)[0]


def test_torque_free_rotation():
    n = 200
    inertia = np.array([[2500.0, 30.0, -12.0], [30.0, 3100.0, 45.0], [-12.0, 45.0, 2800.0]])
    dyn = RigidDynamics(mass=1.0, inertia=inertia, centre=(0, 0, 0), orientation=tilted(), angular_velocity=(0.04, -0.03, 0.06))
    poses, states = run(dyn, np.zeros((n, 6)))
    assert np.array_equal(states[:, 10:13], np.tile(states[0, 10:13], (n + 1, 1)))  # L is bit-constant
    norm = np.sqrt((states[:, 6:10] ** 2).sum(axis=1))
    print(f"max | |q| - 1 | {np.abs(norm - 1).max():.3e} (bound {dref.QUAT_NORM_BOUND:.3e})")
    assert np.abs(norm - 1.0).max() <= dref.QUAT_NORM_BOUND
    R = poses[:, 0:9].reshape(-1, 3, 3)
    ortho = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max()
    print(f"max |R^T R - I| {ortho:.3e} (bound {dref.ORTHO_BOUND:.3e})")
    assert ortho <= dref.ORTHO_BOUND
    assert np.abs(R[-1] - R[0]).max() > 0.5  # (it did turn: about 15 radians)
    # the reported w is R Ib^-1 R^T L of the same row
    for t in (0, n):
        assert np.allclose(R[t] @ np.linalg.inv(inertia) @ R[t].T @ states[t, 10:13], poses[t, 12:15], rtol=1e-13, atol=0)
    assert np.allclose(poses[0, 12:15], (0.04, -0.03, 0.06), rtol=1e-13, atol=0)


def test_isotropic_inertia_turns_at_a_constant_rate():
    """Isotropic inertia: w = L / I whatever R is.  About a coordinate axis and with dyadic values every product that enters
    w = R (Iinv (R^T L)) is a product with an exact 0 or 1, so w is bit-constant; R(n) is the n-th power of the one-step Cayley
    rotation (angle 2 atan(|w| / 2) about w / |w|) up to rounding: each step multiplies by a rotation that carries at most
    ORTHO_BOUND of error and errors of rotations add up, so |R(n) - C^n| <= n ORTHO_BOUND."""
    n = 64
    dyn = RigidDynamics(mass=1.0, inertia=8.0, centre=(0, 0, 0), angular_velocity=(0.0, 0.0, 0.125))
    poses, states = run(dyn, np.zeros((n, 6)))
    assert np.array_equal(poses[:, 12:15], np.tile([0.0, 0.0, 0.125], (n + 1, 1)))
    angle = 2.0 * np.arctan(0.125 / 2.0)
    for t in (1, 7, n):
        c, s = np.cos(t * angle), np.sin(t * angle)
        err = np.abs(poses[t, 0:9].reshape(3, 3) - np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])).max()
        assert err <= t * dref.ORTHO_BOUND, (t, err)
    # a general direction: w stays w0 within the rounding of the three matrix products (a few ulp), not bit for bit
    w0 = np.array([0.04, -0.03, 0.06])
    dyn = RigidDynamics(mass=1.0, inertia=8.0, centre=(0, 0, 0), orientation=tilted(), angular_velocity=w0)
    poses, _ = run(dyn, np.zeros((n, 6)))
    assert np.abs(poses[:, 12:15] - w0).max() <= dref.ORTHO_BOUND * np.abs(w0).max()
    C = RigidMotion((0, 0, 0), w0, 0.0, phase=2.0 * np.arctan(np.sqrt((w0 * w0).sum()) / 2.0)).at(0)[0]
    assert np.abs(poses[n, 0:9].reshape(3, 3) - np.linalg.matrix_power(C, n) @ tilted()).max() <= n * dref.ORTHO_BOUND


def test_axis_mode():
    n = 32
    a = np.array([0.0, 3.0, 4.0]) / 5.0
    inertia = np.diag([4.0, 8.0, 16.0])
    I_a = float(a @ inertia @ a)
    dyn = RigidDynamics(mass=1.0, inertia=inertia, centre=(0, 0, 0), angular_velocity=0.0625 * a, torque=(0.0, 0.25, 0.0), rotate=("axis", 5.0 * a))
    rotate, P, S = dyn.native()
    assert rotate == dref.AXIS and np.array_equal(P[28:31], a) and P[31] == 1.0 / I_a and S[10] == 0.0625
    poses, states = dref.replay(rotate, P, S, np.zeros((n, 6)))
    T = float(a @ np.array([0.0, 0.25, 0.0]))
    rate = 0.0625
    for t in range(n + 1):
        assert states[t, 10] == rate
        assert np.array_equal(poses[t, 12:15], rate * a)
        assert np.abs(poses[t, 0:9].reshape(3, 3) @ a - a).max() <= dref.ORTHO_BOUND  # R fixes the axis
        rate = rate + T * (1.0 / I_a)
    assert np.isclose(states[n, 10], 0.0625 + n * T / I_a, rtol=1e-14, atol=0)
    # loads perpendicular to the axis do nothing
    perp = np.zeros((n, 6))
    perp[:, 3:6] = np.cross(a, (1.0, 0.0, 0.0)) * 3.0
    _, s2 = dref.replay(rotate, P, S, perp)
    assert np.abs(s2[:, 10] - states[:, 10]).max() <= 1e-15 * n


def test_a_load_that_is_not_finite_is_refused():
    dyn = RigidDynamics(mass=2.0, inertia=3.0, centre=(1.0, 2.0, 3.0))
    rotate, P, S = dyn.native()
    for bad in (np.nan, np.inf):
        H = ZERO.copy()
        H[4] = bad
        new, ok = dref.integrate(rotate, P, S, H)
        assert not ok and np.array_equal(new, S)


@pytest.mark.parametrize("kw,word", [
    (dict(mass=0.0), "mass"), (dict(mass=-1.0), "mass"), (dict(mass=np.nan), "mass"), (dict(mass=np.inf), "mass"),
    (dict(inertia=0.0), "inertia"), (dict(inertia=[[1, 2, 0], [0, 1, 0], [0, 0, 1]]), "inertia"), (dict(inertia=np.diag([1.0, -1.0, 1.0])), "inertia"),
    (dict(inertia=[[1, 2, 0], [2, 1, 0], [0, 0, 1]]), "inertia"), (dict(inertia=np.nan), "inertia"), (dict(inertia=np.ones(3)), "inertia"),
    (dict(centre=(0.0, np.inf, 0.0)), "centre"), (dict(velocity=(np.nan, 0, 0)), "velocity"), (dict(angular_velocity=(0, 0, np.inf)), "angular_velocity"),
    (dict(force=(0, np.nan, 0)), "force"), (dict(torque=(0, np.nan, 0)), "torque"), (dict(orientation=np.full((3, 3), np.nan)), "orientation"),
    (dict(orientation=2.0 * np.eye(3)), "orientation"), (dict(spring=((0, 0, 0), np.nan, 0.0)), "spring"), (dict(spring=((0, 0, np.inf), 1.0, 0.0)), "spring"),
    (dict(spring=(1.0, 2.0)), "spring"), (dict(rotate=("axis", (0.0, 0.0, 0.0))), "axis"), (dict(rotate=("axis", (0.0, np.nan, 1.0))), "axis"),
    (dict(rotate="spin"), "rotate"), (dict(translate=(True, False)), "translate"),
])
def test_rigid_dynamics_names_the_bad_argument(kw, word):
    args = dict(mass=1.0, inertia=1.0, centre=(0.0, 0.0, 0.0))
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        RigidDynamics(**args)


def test_sphere_and_body_arguments():
    r, density, g = 5.3, 2.5, np.array([0.0, 0.0, -2.0**-10])
    V = 4.0 / 3.0 * np.pi * r**3
    for make in (RigidDynamics.sphere, RigidDynamics.uhlmann):
        dyn = make(r, density, (1.0, 2.0, 3.0), gravity=g, velocity=(0.0, 0.0, 0.01), rotate="locked")
        assert np.isclose(dyn.mass, 1.5 * V, rtol=1e-15) and np.allclose(dyn.inertia, 1.5 * 0.4 * V * r * r * np.eye(3), rtol=1e-15)
        assert np.allclose(dyn.force, 1.5 * V * g, rtol=1e-15) and dyn.rotate == RigidDynamics.ROTATE_LOCKED and dyn.velocity[2] == 0.01
        for light in (1.2, 1.0, 0.5):
            with pytest.raises(ValueError, match="density"):
                make(r, light, (1.0, 2.0, 3.0))
    assert "unstable" in RigidDynamics.sphere.__doc__
    dyn = RigidDynamics(mass=1.0, inertia=1.0, centre=(4.0, 5.0, 6.0))
    with pytest.raises(TypeError, match="mutually exclusive"):
        IBMBody(slice(0, 10), motion=RigidMotion((0, 0, 0), (0, 0, 1), 0.1), dynamics=dyn)
    with pytest.raises(TypeError, match="RigidDynamics"):
        IBMBody(slice(0, 10), dynamics="free")
    body = IBMBody(slice(0, 10), dynamics=dyn)
    assert body.motion is None and body.dynamics is dyn and body.centre0 is None
    # the quaternion handed to the device is the orientation's, in every branch of the conversion
    for axis, angle in (((1.0, 2.0, -0.5), 0.7), ((1, 0, 0), 3.1), ((0, 1, 0), 3.1), ((0, 0, 1), 3.1), ((1, 1, 1), 2.0)):
        R0 = RigidMotion((0, 0, 0), axis, 0.0, phase=angle).at(0)[0]
        q = RigidDynamics(mass=1.0, inertia=1.0, centre=(0, 0, 0), orientation=R0).native()[2][6:10]
        assert np.abs(np.array(dref.quat_matrix(q)).reshape(3, 3) - R0).max() <= 1e-15


def test_sanity_pin_of_the_coupled_case():
    """The restatement alone, FP32FP32 D3Q19 BGK (the case and the choice of gravity: tests/_ibm_dynamics_ref.py): every marker's
    support stays inside the box, |v| <= 0.03, and at every row 0 > v_z > -(t + 1) |force_z| / mass — the reaction opposes the fall
    and does not reverse it.  From the second row on the body is also slower than its own free fall, v_z(0) - t |force_z| / mass."""
    lat = orc.Lattice("D3Q19")
    X0 = ref.fibonacci_sphere(dref.N_MARKERS, dref.RADIUS, dref.CENTRE)
    areas = np.full(dref.N_MARKERS, 4 * np.pi * dref.RADIUS**2 / dref.N_MARKERS, dtype=np.float32)
    dyn = RigidDynamics.sphere(dref.RADIUS, dref.DENSITY, dref.CENTRE, gravity=(0, 0, -dref.GRAVITY), velocity=(0, 0, -dref.GRAVITY / 2))
    out = dref.coupled_run(dyn, X0, areas, orc.initialize_eq(dref.SHAPE, lat, "FP32FP32"), lat, "FP32FP32", "BGK")
    poses = out["poses"]
    assert poses.shape == (dref.COUPLED_STEPS + 1, 18)
    dref.check_fall(poses, dyn)
    X = out["positions"]
    assert X.min() - 2.0 >= 0.0 and X.max() + 2.0 <= 24.0
    assert np.abs(out["forces"]).max() > 1e-6 and out["sweeps"] == 2

