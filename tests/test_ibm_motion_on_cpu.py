"""The rigid-body kernels of the immersed-boundary stepper without a GPU: xlb_amd/csrc/ibm_motion_kernels.hpp compiled for the host
(tests/hip_on_cpu stands in for the HIP runtime header, tests/ibm_motion_cpu_emulation.cpp builds the tables of
xlbhip_ibm_set_bodies and launches the kernels one emulated thread after the other) against tests/_ibm_motion_ref.py.  This checks
the kernels' arithmetic, indexing and the fixed summation order — not the GPU's code generation, which tests/test_gpu_ibm_motion.py
covers."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from xlb_amd.helper.ibm_helper import RigidMotion

import _ibm_motion_ref as mref
import _ibm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOTION = RigidMotion(centre=(9.0, 10.0, 11.85), axis=(0, 0, 1), rate=0.008, velocity=(0.02, 0.01, -0.005))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("ibm_motion_cpu") / "libibm_motion_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", os.path.join(ROOT, "tests", "ibm_motion_cpu_emulation.cpp"), "-o", str(so)],
                   check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.move_cpu.argtypes = [C.c_int64, C.c_int] + [C.c_void_p] * 8
    lib.loads_cpu.argtypes = [C.c_int64, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 5
    return lib


def ptr(a):
    return a.ctypes.data


def pose_rows(bodies, t):
    """[n_bodies][18] as IBMStepper stages them: R | c | w | v, the identity about centre0 for a body at rest."""
    rows = np.zeros((len(bodies), 18))
    for i, (_, motion, centre0) in enumerate(bodies):
        R, c, w, v = (np.eye(3), np.asarray(centre0, np.float64), np.zeros(3), np.zeros(3)) if motion is None else mref.pose(motion, t)
        rows[i] = np.concatenate([R.reshape(9), c, w, v])
    return rows


def body_arrays(bodies):
    first = np.array([sl.start for sl, _, _ in bodies], np.int64)
    count = np.array([sl.stop - sl.start for sl, _, _ in bodies], np.int64)
    moving = np.array([m is not None for _, m, _ in bodies], np.int32)
    centre0 = np.ascontiguousarray([c for _, _, c in bodies], np.float64)
    return first, count, moving, centre0


def test_move_matches_the_restatement_bit_for_bit(lib):
    """Two bodies — markers 20 .. 270 moving, 300 .. 390 at rest — and markers in no body (0 .. 20, 270 .. 300, 390 .. 400)."""
    X0 = ref.fibonacci_sphere(400, 5.3, (11.3, 12.6, 11.85))
    U0 = np.random.default_rng(1).normal(scale=0.01, size=X0.shape).astype(np.float32)
    bodies = [(slice(20, 270), MOTION, MOTION.at(0)[1]), (slice(300, 390), None, X0[300:390].astype(np.float64).mean(axis=0))]
    first, count, moving, centre0 = body_arrays(bodies)
    for t in (0, 5, 11):
        pose = pose_rows(bodies, t)
        pos, vel = X0.copy(), U0.copy()
        assert lib.move_cpu(400, 2, ptr(first), ptr(count), ptr(moving), ptr(centre0), ptr(pose), ptr(X0), ptr(pos), ptr(vel)) == 0
        X, U = mref.move_bodies(X0, U0, bodies, t)
        assert np.array_equal(pos, X) and np.array_equal(vel, U), t
        untouched = np.r_[0:20, 270:400]
        assert np.array_equal(pos[untouched], X0[untouched]) and np.array_equal(vel[untouched], U0[untouched])
        assert (t == 0) == np.array_equal(pos[20:270], X0[20:270])  # the body does move
        assert not np.array_equal(vel[20:270], U0[20:270])  # the uploaded velocities of a moving body are ignored


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_loads_within_the_derived_bound_and_reproducible(lib, dtype):
    """Bodies of 250 markers (one chunk, partly filled), 700 (three chunks), 256 (exactly one) and 1, not in array order; a gap of
    markers in no body.  The kernel's tree against the sequential double sum: within 2 n 2^-53 sum |term| per component — and the
    tree restated in NumPy with every level's additions done at once (what the parallel kernel does): the same bits."""
    rng = np.random.default_rng(11)
    n = 1300
    F = np.ascontiguousarray(rng.normal(scale=2e-3, size=(n, 3)).astype(dtype))
    A = rng.uniform(0.5, 1.5, n).astype(np.float32)
    X = rng.uniform(5.0, 19.0, (n, 3)).astype(np.float32)
    ranges = [slice(300, 1000), slice(0, 250), slice(1040, 1296), slice(1299, 1300)]
    first = np.array([s.start for s in ranges], np.int64)
    count = np.array([s.stop - s.start for s in ranges], np.int64)
    pose = np.zeros((4, 18))
    pose[:, 9:12] = rng.uniform(9.0, 13.0, (4, 3))
    out = []
    for _ in range(2):
        loads, row = np.full((4, 6), np.nan), np.full((4, 6), np.nan)
        assert lib.loads_cpu(n, 4, ptr(first), ptr(count), ptr(pose), int(dtype == np.float32), ptr(F), ptr(A), ptr(X), ptr(loads), ptr(row)) == 0
        assert np.array_equal(loads, row)  # the history row carries the same values
        out.append(loads)
    assert np.array_equal(out[0], out[1])
    for b, sl in enumerate(ranges):
        c = pose[b, 9:12]
        exp, bound = mref.loads(F[sl], A[sl], X[sl], c), mref.loads_bound(F[sl], A[sl], X[sl], c)
        err = np.abs(out[0][b] - exp)
        print(f"body {b} ({count[b]} markers): max |d| {err.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}, |load| {np.abs(exp).max():.3e}")
        assert (err <= bound).all(), (b, err, bound)
        assert count[b] == 1 or np.abs(exp).max() > 1e-4
        assert np.array_equal(out[0][b], mref.loads_tree(F[sl], A[sl], X[sl], c))
    # no history row asked for
    loads = np.zeros((4, 6))
    assert lib.loads_cpu(n, 4, ptr(first), ptr(count), ptr(pose), int(dtype == np.float32), ptr(F), ptr(A), ptr(X), ptr(loads), None) == 0
    assert np.array_equal(loads, out[0])
