"""The free-body kernels of the immersed-boundary stepper without a GPU: xlb_amd/csrc/ibm_dynamics_kernels.hpp compiled for the host
(tests/hip_on_cpu stands in for the HIP runtime header, tests/ibm_dynamics_cpu_emulation.cpp launches the kernels one emulated
thread after the other) against tests/_ibm_dynamics_ref.py.  This checks the kernels' arithmetic, operation order and indexing —
not the GPU's code generation (fp64 division and square root), which tests/test_gpu_ibm_dynamics.py covers."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from xlb_amd.helper.ibm_helper import RigidDynamics, RigidMotion

import _ibm_dynamics_ref as dref
import _ibm_motion_ref as mref
import _ibm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 20


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("ibm_dynamics_cpu") / "libibm_dynamics_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", os.path.join(ROOT, "tests", "ibm_dynamics_cpu_emulation.cpp"), "-o", str(so)],
                   check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.pose_cpu.argtypes = [C.c_int] + [C.c_void_p] * 8
    lib.integrate_cpu.argtypes = [C.c_int] + [C.c_void_p] * 6
    lib.move_live_cpu.argtypes = [C.c_int64] + [C.c_void_p] * 6
    return lib


def ptr(a):
    return a.ctypes.data


def bodies():
    """A free body with an anisotropic inertia, tilted and spinning; an axis-mode body on a damped spring that may only move along
    x and z; a prescribed body."""
    tilt = RigidMotion((0, 0, 0), (1.0, 2.0, -0.5), 0.7).at(1)[0]
    free = RigidDynamics(mass=310.0, inertia=[[2500.0, 30.0, -12.0], [30.0, 3100.0, 45.0], [-12.0, 45.0, 2800.0]], centre=(9.1, 10.2, 11.3),
                         velocity=(0.01, -0.02, 0.005), orientation=tilt, angular_velocity=(0.004, -0.003, 0.006), force=(0.0, 0.0, -0.3),
                         torque=(0.2, 0.0, -0.1))
    rotor = RigidDynamics(mass=120.0, inertia=np.diag([900.0, 1100.0, 1300.0]), centre=(14.0, 9.0, 12.5), angular_velocity=(0.0, 0.002, 0.004),
                          spring=((14.5, 9.0, 12.0), (0.8, 0.0, 1.1), 0.05), translate=(True, False, True), rotate=("axis", (0.0, 1.0, 2.0)))
    motion = RigidMotion(centre=(9.0, 10.0, 11.85), axis=(0, 0, 1), rate=0.008, velocity=(0.02, 0.01, -0.005))
    return free, rotor, motion


def tables():
    free, rotor, motion = bodies()
    kind = np.array([2, 2, 1], np.int32)
    rotate, params, state = np.zeros(3, np.int32), np.zeros((3, 32)), np.zeros((3, 16))
    for i, dyn in enumerate((free, rotor)):
        rotate[i], params[i], state[i] = dyn.native()
    rest = np.zeros((3, 18))
    rest[:, 0] = rest[:, 4] = rest[:, 8] = 1.0
    rest[:, 9:12] = [free.centre, rotor.centre, motion.centre]
    return kind, rotate, params, state, rest, motion


def staged_rows(motion, t):
    rows = np.zeros((3, 18))
    rows[:, 0] = rows[:, 4] = rows[:, 8] = 1.0  # (the rows of the dynamic bodies: anything, they are not read)
    R, c, w, v = mref.pose(motion, t)
    rows[2] = np.concatenate([R.reshape(9), c, w, v])
    return rows


def test_poses_and_states_match_the_restatement_bit_for_bit(lib):
    kind, rotate, params, state, rest, motion = tables()
    loads = np.random.default_rng(5).normal(scale=0.4, size=(STEPS, 3, 6))
    exp = [dref.replay(int(rotate[b]), params[b], state[b], loads[:, b]) for b in range(2)]
    status = np.zeros(1, np.uint64)
    initial = state.copy()
    for t in range(STEPS + 1):
        staged = staged_rows(motion, t)
        live, hist = np.full((3, 18), np.nan), np.full((3, 18), np.nan)
        assert lib.pose_cpu(3, ptr(kind), ptr(rotate), ptr(state), ptr(params), ptr(staged), ptr(rest), ptr(live), ptr(hist)) == 0
        assert np.array_equal(live, hist)
        for b in range(2):
            assert np.array_equal(live[b], exp[b][0][t]), (t, b)
            assert np.array_equal(state[b], exp[b][1][t]), (t, b)
        assert np.array_equal(live[2], staged[2])  # the prescribed body's live row is the staged row
        # no history row asked for, nothing staged: the prescribed body falls back to its rest pose
        live2 = np.full((3, 18), np.nan)
        assert lib.pose_cpu(3, ptr(kind), ptr(rotate), ptr(state), ptr(params), None, ptr(rest), ptr(live2), None) == 0
        assert np.array_equal(live2[:2], live[:2]) and np.array_equal(live2[2], rest[2])
        if t < STEPS:
            assert lib.integrate_cpu(3, ptr(kind), ptr(rotate), ptr(params), ptr(loads[t]), ptr(state), ptr(status)) == 0
    assert status[0] == 0
    assert np.array_equal(state[2], initial[2])  # a prescribed body has no state to advance
    # the bodies did move and turn, the constrained axis did not
    assert not np.array_equal(exp[0][0][0][:9], exp[0][0][-1][:9]) and not np.array_equal(exp[1][0][0][:9], exp[1][0][-1][:9])
    assert np.array_equal(exp[1][1][:, 1], np.full(STEPS + 1, 9.0)) and np.abs(exp[1][1][-1, 0] - 14.0) > 1e-3
    axis = params[1, 28:31]
    for row in exp[1][0]:
        assert np.abs(row[:9].reshape(3, 3) @ axis - axis).max() <= dref.ORTHO_BOUND  # the axis-mode body turns about its axis only


def test_a_nan_load_stops_exactly_that_body(lib):
    kind, rotate, params, state, rest, motion = tables()
    loads = np.random.default_rng(6).normal(scale=0.4, size=(3, 6))
    for bad, column in ((0, 4), (1, 2), (1, 3)):
        S, status = state.copy(), np.zeros(1, np.uint64)
        H = loads.copy()
        H[bad, column] = np.nan
        assert lib.integrate_cpu(3, ptr(kind), ptr(rotate), ptr(params), ptr(H), ptr(S), ptr(status)) == 0
        assert status[0] == 1 << bad
        assert np.array_equal(S[bad], state[bad])
        other = 1 - bad
        assert np.array_equal(S[other], dref.integrate(int(rotate[other]), params[other], state[other], H[other])[0])
        assert not np.array_equal(S[other], state[other])
        assert dref.integrate(int(rotate[bad]), params[bad], state[bad], H[bad])[1] is False
        # sticky: a good step afterwards keeps the bit and moves the body again
        assert lib.integrate_cpu(3, ptr(kind), ptr(rotate), ptr(params), ptr(loads), ptr(S), ptr(status)) == 0
        assert status[0] == 1 << bad and not np.array_equal(S[bad], state[bad])
    # an overflow is caught like a NaN
    S, status = state.copy(), np.zeros(1, np.uint64)
    H = loads.copy()
    H[0, 0] = 1e308 * 310.0
    assert lib.integrate_cpu(3, ptr(kind), ptr(rotate), ptr(params), ptr(H), ptr(S), ptr(status)) == 0
    assert status[0] == 1 and np.array_equal(S[0], state[0])


def test_move_reads_the_live_table(lib):
    """Markers 20 .. 270 the free body, 300 .. 390 the prescribed one, the others in no body: placed from the live rows as
    tests/_ibm_motion_ref.py places them from the same poses, the markers in no body untouched."""
    kind, rotate, params, state, rest, motion = tables()
    kind, rotate, params, state, rest = (np.ascontiguousarray(a[[0, 2]]) for a in (kind, rotate, params, state, rest))
    X0 = ref.fibonacci_sphere(400, 5.3, (11.3, 12.6, 11.85))
    U0 = np.random.default_rng(1).normal(scale=0.01, size=X0.shape).astype(np.float32)
    move_id = np.full(400, -1, np.int32)
    move_id[20:270], move_id[300:390] = 0, 1
    centre0 = np.ascontiguousarray([state[0, 0:3], motion.centre])
    staged = np.ascontiguousarray(staged_rows(motion, 3)[[0, 2]])
    live = np.zeros((2, 18))
    assert lib.pose_cpu(2, ptr(kind), ptr(rotate), ptr(state), ptr(params), ptr(staged), ptr(rest), ptr(live), None) == 0
    pos, vel = X0.copy(), U0.copy()
    assert lib.move_live_cpu(400, ptr(move_id), ptr(centre0), ptr(live), ptr(X0), ptr(pos), ptr(vel)) == 0
    for b, sl in enumerate((slice(20, 270), slice(300, 390))):
        P = live[b]
        X, V = mref.move(X0[sl], centre0[b], P[:9].reshape(3, 3), P[9:12], P[12:15], P[15:18])
        assert np.array_equal(pos[sl], X) and np.array_equal(vel[sl], V)
        assert not np.array_equal(pos[sl], X0[sl])
    untouched = np.r_[0:20, 270:300, 390:400]
    assert np.array_equal(pos[untouched], X0[untouched]) and np.array_equal(vel[untouched], U0[untouched])
