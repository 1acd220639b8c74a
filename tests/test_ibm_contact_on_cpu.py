"""Virtual mass and contact forces of the free bodies without a GPU: closed forms of the restatement tests/_ibm_contact_ref.py, the
kernel k_ibm_integrate_contact compiled for the host (tests/ibm_contact_cpu_emulation.cpp through tests/hip_on_cpu) against it bit
for bit, the stability of the coupled restatement with and without a virtual mass, and the argument checks."""

import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.helper.ibm_helper import IBMBody, RigidDynamics, RigidMotion

import _ibm_contact_ref as cref
import _ibm_dynamics_ref as dref
import _ibm_motion_ref as mref
import _ibm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 20
INERTIA = np.array([[2500.0, 30.0, -12.0], [30.0, 3100.0, 45.0], [-12.0, 45.0, 2800.0]])


def tilted():
    return RigidMotion((0, 0, 0), (1.0, 2.0, -0.5), 0.7).at(1)[0]


def run(dyn, loads):
    """One body, no contact -> (states (n + 1, 16), prevs (n + 1, 6))"""
    rotate, P, S = dyn.native()
    _, states, prevs, _ = cref.replay([2], [rotate], P[None], S[None], np.asarray(loads)[:, None], np.array([dyn.virtual()]))
    return states[:, 0], prevs[:, 0]


# ---- closed forms -----------------------------------------------------------------------------------------------------------------
def dyadic(n):
    return 1.0 - 0.5 ** np.arange(1, n + 1)  # 1/2, 3/4, 7/8, ...: exact in fp64


def test_constant_force_gives_dyadic_accelerations():
    """m = 1, m_v = 1, F = 1: a_n = (1 + a_{n-1}) / 2 = 1 - 2^-n exactly, converging to F / m."""
    n = 40
    dyn = RigidDynamics(mass=1.0, inertia=1.0, centre=(0, 0, 0), force=(1.0, 0.0, 0.0), rotate="locked", virtual_mass=1.0)
    states, prevs = run(dyn, np.zeros((n, 6)))
    assert np.array_equal(prevs[1:, 0], dyadic(n)) and np.array_equal(prevs[:, 1:], np.zeros((n + 1, 5)))
    assert np.array_equal(states[1:, 3], np.cumsum(dyadic(n))) and np.array_equal(states[1:, 0], np.cumsum(np.cumsum(dyadic(n))))
    assert abs(prevs[-1, 0] - 1.0) < 1e-11
    # a masked axis: translate = 0 stores a_prev = 0 and the body does not move
    dyn = RigidDynamics(mass=1.0, inertia=1.0, centre=(0, 0, 0), force=(1.0, 0.0, 0.0), rotate="locked", virtual_mass=1.0, translate=(False, True, True))
    states, prevs = run(dyn, np.zeros((5, 6)))
    assert np.array_equal(prevs, np.zeros((6, 6))) and np.array_equal(states[:, 0:6], np.zeros((6, 6)))


@pytest.mark.parametrize("rotate", [("axis", (0.0, 0.0, 1.0)), "free"])
def test_constant_torque_gives_dyadic_angular_accelerations(rotate):
    """Isotropic I = 1, I_v = 1, torque 1 about z: every product in w = R (Iinv (R^T L)) of a rotation about z is one with an exact
    0, 1 or 1/2, so alpha_n = 1 - 2^-n exactly in both modes."""
    n = 20
    dyn = RigidDynamics(mass=1.0, inertia=1.0, centre=(0, 0, 0), torque=(0.0, 0.0, 1.0), rotate=rotate, virtual_inertia=1.0)
    states, prevs = run(dyn, np.zeros((n, 6)))
    assert np.array_equal(prevs[1:, 5], dyadic(n)) and np.array_equal(prevs[:, :5], np.zeros((n + 1, 5)))
    rate = states[:, 10] if rotate != "free" else states[:, 12] / 2.0  # (free: L_z = (I + I_v) w_z)
    assert np.array_equal(rate[1:], np.cumsum(dyadic(n)))
    assert np.abs(np.sqrt((states[:, 6:10] ** 2).sum(axis=1)) - 1.0).max() <= dref.QUAT_NORM_BOUND


def test_torque_free_rotation_with_a_virtual_inertia():
    # isotropic, about a coordinate axis, dyadic values: the rate is kept bit for bit (as without I_v) and alpha_prev stays zero
    n = 64
    dyn = RigidDynamics(mass=1.0, inertia=6.0, centre=(0, 0, 0), angular_velocity=(0.0, 0.0, 0.125), virtual_inertia=2.0)
    rotate, P, S = dyn.native()
    poses, states, prevs, _ = cref.replay([2], [rotate], P[None], S[None], np.zeros((n, 1, 6)), np.array([dyn.virtual()]))
    assert np.array_equal(poses[:, 0, 12:15], np.tile([0.0, 0.0, 0.125], (n + 1, 1))) and np.array_equal(prevs, np.zeros((n + 1, 1, 6)))
    plain = RigidDynamics(mass=1.0, inertia=8.0, centre=(0, 0, 0), angular_velocity=(0.0, 0.0, 0.125))
    assert np.array_equal(poses[:, 0], dref.replay(*plain.native(), np.zeros((n, 6)))[0])
    # anisotropic: L (and with it |L|) is bit-constant, as tests/test_ibm_dynamics_host.py::test_torque_free_rotation demands
    n = 200
    dyn = RigidDynamics(mass=1.0, inertia=INERTIA, centre=(0, 0, 0), orientation=tilted(), angular_velocity=(0.04, -0.03, 0.06), virtual_inertia=700.0)
    states, prevs = run(dyn, np.zeros((n, 6)))
    assert np.array_equal(states[:, 10:13], np.tile(states[0, 10:13], (n + 1, 1))) and np.array_equal(prevs, np.zeros((n + 1, 6)))
    assert np.abs(np.sqrt((states[:, 6:10] ** 2).sum(axis=1)) - 1.0).max() <= dref.QUAT_NORM_BOUND
    assert np.abs(states[-1, 6:10] - states[0, 6:10]).max() > 0.1  # (it did turn)


def three_bodies():
    """The bodies of tests/test_ibm_dynamics_on_cpu.py."""
    free = RigidDynamics(mass=310.0, inertia=INERTIA, centre=(9.1, 10.2, 11.3), velocity=(0.01, -0.02, 0.005), orientation=tilted(),
                         angular_velocity=(0.004, -0.003, 0.006), force=(0.0, 0.0, -0.3), torque=(0.2, 0.0, -0.1))
    rotor = RigidDynamics(mass=120.0, inertia=np.diag([900.0, 1100.0, 1300.0]), centre=(14.0, 9.0, 12.5), angular_velocity=(0.0, 0.002, 0.004),
                          spring=((14.5, 9.0, 12.0), (0.8, 0.0, 1.1), 0.05), translate=(True, False, True), rotate=("axis", (0.0, 1.0, 2.0)))
    locked = RigidDynamics(mass=50.0, inertia=10.0, centre=(3.0, 4.0, 5.0), velocity=(0.0, 0.01, 0.0), force=(-0.0, 0.1, 0.0), rotate="locked")
    return free, rotor, locked


def test_without_virtual_mass_and_contact_it_is_the_plain_integrator():
    loads = np.random.default_rng(5).normal(scale=0.4, size=(STEPS, 6))
    for dyn in three_bodies():
        rotate, P, S = dyn.native()
        assert dyn.virtual() == (0.0, 0.0)
        states, _ = run(dyn, loads)
        assert np.array_equal(states, dref.replay(rotate, P, S, loads)[1])


# ---- contact ----------------------------------------------------------------------------------------------------------------------
def test_two_bodies_bounce_off_each_other():
    """Two equal spheres (m = 1000, r = 2) approach along x at +-u0 / 2 with zero loads; zeta = 0.25, k = 0.1.

    The energy bound.  In the relative coordinate (separation s, relative velocity u, overlap p = zeta - (s - 2 r), force
    f(p) = k p^2, potential Phi(p) = k p^3 / 3, energy E = m u^2 / 4 + Phi) one step of the scheme, dt = 1, is u' = u + 2 f / m,
    p' = p - u'.  Then m (u'^2 - u^2) / 4 = f (u + u') / 2 and, by Taylor with some eta between p and p',
    Phi(p') - Phi(p) = -f u' + f'(eta) u'^2 / 2, so E' - E = -f^2 / m + f'(eta) u'^2 / 2 and, with f' = 2 k p,
    |E' - E| <= f_max^2 / m + k p_max u_max^2 per step in range.  Before and after the bounce Phi = 0, so the kinetic energies
    differ by at most N (f_max^2 / m + k p_max u_max^2), N the steps in range, p_max and u_max the largest overlap and relative
    speed the run met (rounding, 1e-16 relative per operation, is far below).  The parameters make the contact slow against the
    step (about 700 steps in range), so that this is a few per cent of the energy."""
    m, r, zeta, k, u0 = 1000.0, 2.0, 0.25, 0.1, 5e-4
    gap0 = 0.26
    x = r + gap0 / 2.0
    make = lambda sign: RigidDynamics(mass=m, inertia=1.0, centre=(sign * x, 0.0, 0.0), velocity=(-sign * u0 / 2.0, 0.0, 0.0), rotate="locked")  # noqa: E731
    natives = [make(-1.0).native(), make(1.0).native()]
    P, S = np.array([n[1] for n in natives]), np.array([n[2] for n in natives])
    model = cref.Contact([r, r], zeta, k)
    n = 1200
    _, states, _, contacts = cref.replay([2, 2], [0, 0], P, S, np.zeros((n, 2, 6)), np.zeros((2, 2)), model)
    assert np.array_equal(states[:, 0, 3:6], -states[:, 1, 3:6]) and np.array_equal(states[:, 0, 0:3], -states[:, 1, 0:3])  # exact mirrors
    assert np.array_equal(contacts[:, 0], -contacts[:, 1])
    overlap = zeta - ((states[:, 1, 0] - states[:, 0, 0]) - 2.0 * r)
    u = states[:, 1, 3] - states[:, 0, 3]
    inside = overlap > 0.0
    assert not inside[0] and not inside[-1] and inside.any()  # they met and separated again
    assert u[0] < 0.0 < u[-1] and overlap[-1] < overlap[0]
    assert (np.abs(contacts[:, 0, 0]) > 0.0).sum() == inside[:-1].sum()
    N, p_max, u_max = int(inside.sum()), float(overlap.max()), float(np.abs(u).max())
    bound = N * ((k * p_max * p_max) ** 2 / m + k * p_max * u_max * u_max)
    e0, e1 = m * u[0] ** 2 / 4.0, m * u[-1] ** 2 / 4.0
    print(f"steps in range {N}, largest overlap {p_max:.4f}, kinetic energy {e0:.6e} -> {e1:.6e}, |difference| {abs(e1 - e0):.3e}, bound {bound:.3e}")
    assert bound <= 0.1 * e0  # (the bound says something)
    assert abs(e1 - e0) <= bound


def test_a_body_comes_to_rest_above_a_floor():
    """m = 1000 under the weight W = 0.01 above the plane z = 3, r = 2, zeta = 0.5, k_w = 1: k_w zeta^2 = 0.25 > W.  Released at rest
    0.1 above the range, it enters with the kinetic energy 0.1 W = 0.001; reaching the plane would take the work
    k_w zeta^3 / 3 - W zeta = 0.037: it turns round far above it."""
    m, W, r, zeta, kw, lo = 1000.0, 0.01, 2.0, 0.5, 1.0, 3.0
    dyn = RigidDynamics(mass=m, inertia=1.0, centre=(7.0, 8.0, lo + r + zeta + 0.1), force=(0.0, 0.0, -W), rotate="locked")
    rotate, P, S = dyn.native()
    model = cref.Contact([r], zeta, 0.0, kw, lo=(-np.inf, -np.inf, lo))
    n = 1500
    _, states, _, contacts = cref.replay([2], [rotate], P[None], S[None], np.zeros((n, 1, 6)), np.zeros((1, 2)), model)
    gap = states[:, 0, 2] - (lo + r)
    assert gap.min() > 0.0 and gap.min() < zeta  # in range, never through the plane
    assert (contacts[:, 0, 2] > 0.0).any() and (contacts[:, 0, 2] >= 0.0).all() and np.array_equal(contacts[:, 0, :2], np.zeros((n, 2)))
    assert states[:, 0, 5].max() > 0.0  # it bounced
    assert np.array_equal(states[:, 0, 0:2], np.tile([7.0, 8.0], (n + 1, 1)))


def test_coincident_centres_and_planes_at_infinity():
    C3 = np.array([[5.0, 6.0, 7.0], [5.0, 6.0, 7.0], [5.5, 6.0, 7.0]])
    model = cref.Contact([1.0, 1.0, 0.0], 0.5, 3.0)
    for i in (0, 1):  # d = 0: no force and no NaN; the body without a radius is no obstacle
        assert np.array_equal(cref.contact_force(i, C3, model), np.zeros(3))
    model = cref.Contact([1.0, 1.0, 1.0], 0.5, 3.0)
    F = cref.contact_force(0, C3, model)
    assert np.isfinite(F).all() and F[0] < 0.0 and np.array_equal(F[1:], np.zeros(2))  # only body 2, at d = 0.5, pushes
    one = C3[2:3]
    for lo, hi in ((None, None), ((-np.inf,) * 3, (np.inf,) * 3)):
        F = cref.contact_force(0, one, cref.Contact([1.0], 0.5, 3.0, 2.0, lo=lo, hi=hi))
        assert np.array_equal(F, np.zeros(3)) and not np.signbit(F).any()
    F = cref.contact_force(0, one, cref.Contact([1.0], 0.5, 3.0, 2.0, lo=(4.25, -np.inf, -np.inf), hi=(np.inf, 7.25, np.inf)))
    assert np.array_equal(F, [2.0 * 0.25 * 0.25, -2.0 * 0.25 * 0.25, 0.0])  # gaps 0.25: k_w (zeta - gap)^2, +x from lo, -y from hi


# ---- the kernel on the host ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("ibm_contact_cpu") / "libibm_contact_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", os.path.join(ROOT, "tests", "ibm_contact_cpu_emulation.cpp"), "-o", str(so)],
                   check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.pose_table_cpu.argtypes = [C.c_int] + [C.c_void_p] * 7
    lib.integrate_contact_cpu.argtypes = [C.c_int] + [C.c_void_p] * 12
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def four_bodies():
    """A free body (anisotropic, tilted, spinning) and an axis-mode body on a damped spring, both with virtual mass and inertia and a
    radius of 2, 4.1 apart; a prescribed obstacle 4.1 below the free body; a fourth free body with neither, far away (it must move
    as k_ibm_integrate moves it).  The planes y = 7.9 and x = 15.4 are 0.3 and 0.2 from the first two."""
    free = RigidDynamics(mass=310.0, inertia=INERTIA, centre=(9.1, 10.2, 11.3), velocity=(0.001, -0.002, 0.0005), orientation=tilted(),
                         angular_velocity=(0.004, -0.003, 0.006), force=(0.0, 0.0, -0.3), torque=(0.2, 0.0, -0.1), virtual_mass=500.0, virtual_inertia=900.0)
    rotor = RigidDynamics(mass=120.0, inertia=np.diag([900.0, 1100.0, 1300.0]), centre=(13.2, 10.0, 11.5), angular_velocity=(0.0, 0.002, 0.004),
                          spring=((13.3, 10.0, 11.4), (0.8, 0.0, 1.1), 0.05), translate=(True, False, True), rotate=("axis", (0.0, 1.0, 2.0)),
                          virtual_mass=200.0, virtual_inertia=400.0)
    motion = RigidMotion(centre=(9.0, 10.0, 7.2), axis=(0, 0, 1), rate=0.008, velocity=(0.002, 0.001, 0.003))
    plain = three_bodies()[2]
    kind = np.array([2, 2, 1, 2], np.int32)
    rotate, params, state, virt = np.zeros(4, np.int32), np.zeros((4, 32)), np.zeros((4, 16)), np.zeros((4, 2))
    for i, dyn in ((0, free), (1, rotor), (3, plain)):
        rotate[i], params[i], state[i] = dyn.native()
        virt[i] = dyn.virtual()
    model = cref.Contact([2.0, 2.0, 2.0, 0.0], 0.5, 2.0, 1.5, lo=(-np.inf, 7.9, -np.inf), hi=(15.4, np.inf, np.inf))
    return kind, rotate, params, state, virt, motion, model, plain


def test_kernel_matches_the_restatement_bit_for_bit(lib):
    kind, rotate, params, state, virt, motion, model, plain = four_bodies()
    loads = np.random.default_rng(11).normal(scale=0.4, size=(STEPS, 4, 6))
    staged = np.zeros((STEPS + 1, 4, 18))
    for t in range(STEPS + 1):
        R, c, w, v = mref.pose(motion, t)
        staged[t, 2] = np.concatenate([R.reshape(9), c, w, v])
    poses, states, prevs, contacts = cref.replay(kind, rotate, params, state, loads, virt, model, staged)
    rest = np.zeros((4, 18))
    packed = np.array([model.range, model.stiffness, model.wall_stiffness, *model.lo, *model.hi])
    S, prev, status = state.copy(), np.zeros((4, 6)), np.zeros(1, np.uint64)
    for t in range(STEPS):
        live, contact = np.full((4, 18), np.nan), np.full((4, 3), np.nan)
        assert lib.pose_table_cpu(4, ptr(kind), ptr(rotate), ptr(S), ptr(params), ptr(np.ascontiguousarray(staged[t])), ptr(rest), ptr(live)) == 0
        assert np.array_equal(live, poses[t]), t
        assert lib.integrate_contact_cpu(4, ptr(kind), ptr(rotate), ptr(params), ptr(np.ascontiguousarray(loads[t])), ptr(S), ptr(status), ptr(virt),
                                         ptr(prev), ptr(model.radius), ptr(packed), ptr(live), ptr(contact)) == 0
        assert np.array_equal(S, states[t + 1]), t
        assert np.array_equal(prev, prevs[t + 1]), t
        assert np.array_equal(contact, contacts[t]), t
    assert status[0] == 0
    # every part was exercised: both bodies in contact at every step, from a plane and from a body; the obstacle and the body
    # without a radius got nothing; a_prev and alpha_prev moved
    assert (np.abs(contacts[:, :2]).max(axis=2) > 0.0).all() and np.array_equal(contacts[:, 2:], np.zeros((STEPS, 2, 3)))
    no_planes = cref.Contact(model.radius, model.range, model.stiffness)
    for b, axis in ((0, 1), (1, 0)):  # the plane below the first body in y, the plane beyond the second in x
        pairs_only = cref.contact_force(b, poses[0][:, 9:12], no_planes)
        assert contacts[0, b, axis] != pairs_only[axis] and np.abs(pairs_only).min() > 0.0
    assert np.abs(prevs[-1, 0]).min() > 0.0 and np.abs(prevs[-1, 1, [0, 2, 4, 5]]).min() > 0.0
    assert np.array_equal(prevs[:, 1, 1], np.zeros(STEPS + 1))  # the masked axis
    # the body with neither virtual mass nor a radius: the plain integrator's states
    assert np.array_equal(states[:, 3], dref.replay(int(rotate[3]), params[3], state[3], loads[:, 3])[1])
    # without contact (radius = null) the same bodies move otherwise
    S2, prev2, contact = state.copy(), np.zeros((4, 6)), np.full((4, 3), np.nan)
    live = np.ascontiguousarray(poses[0])
    assert lib.integrate_contact_cpu(4, ptr(kind), ptr(rotate), ptr(params), ptr(np.ascontiguousarray(loads[0])), ptr(S2), ptr(status), ptr(virt), ptr(prev2),
                                     None, ptr(packed), ptr(live), ptr(contact)) == 0
    exp = cref.step_bodies(kind, rotate, params, state, loads[0], virt, np.zeros((4, 6)), poses[0][:, 9:12], None)
    assert np.array_equal(S2, exp[0]) and np.array_equal(prev2, exp[1]) and np.array_equal(contact, np.zeros((4, 3)))
    assert not np.array_equal(S2[:2], states[1][:2])


def test_a_refused_step_leaves_state_and_history_alone(lib):
    kind, rotate, params, state, virt, motion, model, plain = four_bodies()
    packed = np.array([model.range, model.stiffness, model.wall_stiffness, *model.lo, *model.hi])
    loads = np.random.default_rng(12).normal(scale=0.4, size=(4, 6))
    live = np.zeros((4, 18))
    rest = np.zeros((4, 18))
    rest[2, 9:12] = motion.centre
    assert lib.pose_table_cpu(4, ptr(kind), ptr(rotate), ptr(state), ptr(params), None, ptr(rest), ptr(live)) == 0
    S, prev, status, contact = state.copy(), np.zeros((4, 6)), np.zeros(1, np.uint64), np.zeros((4, 3))
    args = lambda H: (4, ptr(kind), ptr(rotate), ptr(params), ptr(H), ptr(S), ptr(status), ptr(virt), ptr(prev), ptr(model.radius), ptr(packed), ptr(live),  # noqa: E731
                      ptr(contact))
    assert lib.integrate_contact_cpu(*args(loads)) == 0 and status[0] == 0
    S1, prev1 = S.copy(), prev.copy()
    bad = loads.copy()
    bad[1, 5] = np.nan
    assert lib.integrate_contact_cpu(*args(bad)) == 0
    assert status[0] == 1 << 1
    assert np.array_equal(S[1], S1[1]) and np.array_equal(prev[1], prev1[1])  # refused: neither the state nor a_prev | alpha_prev
    assert not np.array_equal(S[0], S1[0]) and not np.array_equal(prev[0], prev1[0])  # the other bodies went on
    exp = cref.integrate(int(rotate[1]), params[1], S1[1], bad[1], virt[1], prev1[1], cref.contact_force(1, live[:, 9:12], model))
    assert exp[2] is False and np.array_equal(exp[0], S1[1]) and np.array_equal(exp[1], prev1[1])


# ---- stability of the coupled restatement -----------------------------------------------------------------------------------------
# The sphere of tests/_ibm_dynamics_ref.py (24^3 periodic box, 400 markers, radius 5.3, omega 1.2, D3Q19 BGK FP32FP32, 4 sweeps,
# tolerance 1e-5, relaxation 0.5, rotation locked) under gravity 2^-10 along -z, released at v_z = -g / 2: a gravity at which all four
# sweeps run.  The bands are those of this restatement at EVERY step (profiles/ibm_virtual_mass.md), widened by the stated margins;
# tests/test_gpu_ibm_contact.py holds the device to BAND_LIGHT_START.
G10 = 2.0**-10
BAND_25 = (-2.4656, -2.2382)  # density 2.5, C_v = 4: v_z / g at steps 8 .. 60 (measured -2.4655 .. -2.2383); margin 0.05
BAND_LIGHT = (-0.2464, -0.2264)  # density 1.15, C_v = 8: steps 56 .. 120 (measured -0.2463 .. -0.2265); margin 0.01
BAND_LIGHT_START = (-0.3795, -0.0427)  # the same run, steps 1 .. 12 (measured -0.3795 .. -0.0428); margin 0.01
MARGIN_25, MARGIN_LIGHT = 0.05, 0.01


def coupled_case():
    X0 = ref.fibonacci_sphere(dref.N_MARKERS, dref.RADIUS, dref.CENTRE)
    areas = np.full(dref.N_MARKERS, 4 * np.pi * dref.RADIUS**2 / dref.N_MARKERS, dtype=np.float32)
    return X0, areas


def light_sphere(density, coefficient, **kw):
    return RigidDynamics.sphere(dref.RADIUS, density, dref.CENTRE, gravity=(0, 0, -G10), velocity=(0, 0, -G10 / 2), rotate="locked",
                                virtual_mass_coefficient=coefficient, **kw)


@functools.lru_cache(maxsize=None)
def restated(density, coefficient, steps, policy="FP32FP32"):
    lat = orc.Lattice("D3Q19")
    X0, areas = coupled_case()
    if coefficient > 0:
        dyn = light_sphere(density, coefficient)
    else:  # (sphere() refuses nothing at 2.5, but the point is the body without any virtual term: built directly)
        m = (density - 1.0) * 4.0 / 3.0 * np.pi * dref.RADIUS**3
        dyn = RigidDynamics(mass=m, inertia=m * 0.4 * dref.RADIUS**2, centre=dref.CENTRE, force=(0, 0, -m * G10), velocity=(0, 0, -G10 / 2), rotate="locked")
    return cref.coupled_run(dyn, X0, areas, orc.initialize_eq(dref.SHAPE, lat, policy), lat, policy, "BGK", steps, dref.COUPLED_OMEGA, dref.COUPLED_IBM)


def test_virtual_mass_stabilises_the_coupled_restatement():
    vz = restated(2.5, 4, 60)["poses"][:, 17] / G10
    print("density 2.5, C_v = 4: v_z / g", vz.round(4))
    assert (vz[1:] < 0.0).all() and np.abs(vz).max() < 3.0  # (free fall would be 60)
    assert vz[8:].min() >= BAND_25[0] - MARGIN_25 and vz[8:].max() <= BAND_25[1] + MARGIN_25
    # the same body without the virtual term diverges: the test discriminates
    vz = restated(2.5, 0, 14)["poses"][:, 17] / G10
    print("density 2.5, C_v = 0: v_z / g", vz.round(2))
    assert np.abs(vz).max() > 100.0


def test_a_sphere_of_density_1_15_settles_in_the_restatement():
    vz = restated(1.15, 8, 120)["poses"][:, 17] / G10
    print("density 1.15, C_v = 8: v_z / g", vz.round(4))
    assert np.isfinite(vz).all() and (vz[56:] < 0.0).all()
    assert vz[56:].min() >= BAND_LIGHT[0] - MARGIN_LIGHT and vz[56:].max() <= BAND_LIGHT[1] + MARGIN_LIGHT
    assert vz[1:13].min() >= BAND_LIGHT_START[0] - MARGIN_LIGHT and vz[1:13].max() <= BAND_LIGHT_START[1] + MARGIN_LIGHT


# ---- arguments --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,word", [(dict(virtual_mass=-1.0), "virtual_mass"), (dict(virtual_mass=np.nan), "virtual_mass"),
                                     (dict(virtual_mass=np.inf), "virtual_mass"), (dict(virtual_inertia=-0.5), "virtual_inertia"),
                                     (dict(virtual_inertia=np.inf), "virtual_inertia")])
def test_rigid_dynamics_names_the_bad_virtual_argument(kw, word):
    with pytest.raises(ValueError, match=word):
        RigidDynamics(mass=1.0, inertia=1.0, centre=(0.0, 0.0, 0.0), **kw)


def test_sphere_with_a_coefficient_and_native_tables():
    r, V = 5.3, 4.0 / 3.0 * np.pi * 5.3**3
    for light in (1.2, 1.1):  # without a coefficient the refusal stays
        with pytest.raises(ValueError, match="density must exceed 1.2"):
            RigidDynamics.sphere(r, light, (1.0, 2.0, 3.0))
    for bad in (1.0, 0.9):
        with pytest.raises(ValueError, match="density"):
            RigidDynamics.sphere(r, bad, (1.0, 2.0, 3.0), virtual_mass_coefficient=8.0)
    for bad in (-1.0, np.nan):
        with pytest.raises(ValueError, match="virtual_mass_coefficient"):
            RigidDynamics.sphere(r, 2.5, (1.0, 2.0, 3.0), virtual_mass_coefficient=bad)
    dyn = RigidDynamics.sphere(r, 1.1, (1.0, 2.0, 3.0), virtual_mass_coefficient=8.0, angular_velocity=(0.0, 0.0, 0.01))
    assert np.isclose(dyn.mass, 0.1 * V, rtol=1e-12) and dyn.virtual() == (8.0 * V, 8.0 * 0.4 * V * r * r)
    rotate, P, S = dyn.native()
    assert P.shape == (32,) and S.shape == (16,)
    assert np.isclose(P[0], 1.0 / (8.1 * V), rtol=1e-12) and np.allclose(P[19:28].reshape(3, 3), np.eye(3) / (8.1 * 0.4 * V * r * r), rtol=1e-12)
    assert np.isclose(S[12], 8.1 * 0.4 * V * r * r * 0.01, rtol=1e-12)  # L(0) is the momentum of the inertia WITH the virtual part
    # no virtual quantities: the tables are today's, bit for bit
    a = RigidDynamics(mass=3.0, inertia=INERTIA, centre=(1, 2, 3), orientation=tilted(), angular_velocity=(0.1, 0.2, 0.3), rotate=("axis", (1.0, 1.0, 0.0)))
    b = RigidDynamics(mass=3.0, inertia=INERTIA, centre=(1, 2, 3), orientation=tilted(), angular_velocity=(0.1, 0.2, 0.3), rotate=("axis", (1.0, 1.0, 0.0)),
                      virtual_mass=0.0, virtual_inertia=0.0)
    assert all(np.array_equal(x, y) for x, y in zip(a.native(), b.native()))
    c = RigidDynamics(mass=3.0, inertia=INERTIA, centre=(1, 2, 3), orientation=tilted(), angular_velocity=(0.1, 0.2, 0.3), rotate=("axis", (1.0, 1.0, 0.0)),
                      virtual_mass=1.0, virtual_inertia=100.0)
    assert c.native()[1][0] == 0.25 and c.native()[1][31] < a.native()[1][31] and c.native()[2][10] == a.native()[2][10]


@pytest.mark.parametrize("radius", [0.0, -1.0, np.nan, np.inf])
def test_body_names_a_bad_contact_radius(radius):
    with pytest.raises(ValueError, match="contact_radius"):
        IBMBody(slice(0, 10), contact_radius=radius)
    assert IBMBody(slice(0, 10)).contact_radius is None and IBMBody(slice(0, 10), contact_radius=2).contact_radius == 2.0


@pytest.mark.parametrize("args,kw,word", [((-0.1, 1.0), {}, "range"), ((np.nan, 1.0), {}, "range"), ((0.5, -1.0), {}, "stiffness"),
                                          ((0.5, np.inf), {}, "stiffness"), ((0.5, 1.0), dict(wall_stiffness=-2.0), "wall_stiffness"),
                                          ((0.5, 1.0), dict(wall_stiffness=np.nan), "wall_stiffness"),
                                          ((0.5, 1.0), dict(box=((0.0, 0.0, 5.0), (9.0, 9.0, 5.0))), "lo >= hi along axis 2"),
                                          ((0.5, 1.0), dict(box=((0.0, np.nan, 0.0), (9.0, 9.0, 9.0))), "lo >= hi along axis 1"),
                                          ((0.5, 1.0), dict(box=(0.0, 1.0)), "box")])
def test_set_contact_names_the_bad_argument(args, kw, word):
    """(IBMStepper.set_contact checks its arguments before it touches the device: called on an object that has none)"""
    from xlb_amd.operator.stepper import IBMStepper

    stepper = IBMStepper.__new__(IBMStepper)
    stepper._contact, stepper._any_dynamic, stepper._bodies = None, False, []
    with pytest.raises(ValueError, match=word):
        stepper.set_contact(*args, **kw)
    assert stepper._contact is None
    stepper.set_contact(0.5, 1.0, box=((-np.inf, 2.0, 2.0), (np.inf, 9.0, 9.0)))
    assert stepper._contact[2] == 1.0  # wall_stiffness defaults to stiffness
