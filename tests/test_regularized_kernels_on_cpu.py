"""The regularised collisions without a GPU: xlb_amd/csrc/cell.hpp is compiled for the host (tests/hip_on_cpu stands in for the HIP runtime
header, -ffp-contract=off as in the library's build), tests/regularized_cpu_emulation.cpp runs periodic steps cell by cell through collide<>
with the COLL value the stepper picks, and the populations are compared with the NumPy restatement tests/_regularized_ref.py BIT FOR BIT:
three lattices x both forms x {plain, forced} x the three policies.  Not covered: the step kernel's addressing and boundary rules and the
GPU's code generation (tests/test_gpu_regularized.py)."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _regularized_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE_ID = {"D2Q9": 0, "D3Q19": 1, "D3Q27": 2}
DTYPE_CODE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}  # XLBHIP_F64, XLBHIP_F32
COLLISION_ID = {"RegularizedBGK": 3, "RecursiveRegularizedBGK": 4}
POLICIES = ("FP32FP32", "FP64FP64", "FP64FP32")
SHAPES = {"D2Q9": (6, 5), "D3Q19": (6, 5, 4), "D3Q27": (6, 5, 4)}
OMEGA, STEPS = 1.85, 5


class Case(C.Structure):
    _fields_ = [("f0", C.c_void_p), ("f1", C.c_void_p)] + [(n, C.c_int) for n in ("nx", "ny", "nz", "sdt", "cdt", "collision", "forced")] + [
        ("force", C.c_double * 3), ("omega", C.c_double)]


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("regularized_cpu") / "libregularized_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "regularized_cpu_emulation.cpp"), "-o", str(so)], check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.regularized_cpu.argtypes = [C.c_int, C.POINTER(Case)]
    lib.regularized_operator_cpu.argtypes = [C.c_int, C.POINTER(Case)]
    return lib


def case_of(lat, shape, T, S, form):
    c = Case()
    c.nx, c.ny, c.nz = (1,) * (3 - lat.d) + tuple(shape)
    c.sdt, c.cdt = DTYPE_CODE[np.dtype(S)], DTYPE_CODE[np.dtype(T)]
    c.collision, c.omega = COLLISION_ID[form], OMEGA
    return c


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("forced", [False, True], ids=["plain", "forced"])
@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("lattice", sorted(SHAPES))
def test_emulated_steps_match_the_restatement(emulation, lattice, form, forced, policy):
    lat, shape = orc.Lattice(lattice), SHAPES[lattice]
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    f_0 = ref.sheared_state(shape, lat, policy)
    fv = np.array([1e-4, -2e-4, 3e-4])[: lat.d] if forced else None
    no_bc, no_miss = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    exp = ref.run(f_0, no_bc, no_miss, [], OMEGA, lat, form, STEPS, policy, fv)
    assert np.isfinite(exp).all() and np.abs(exp.astype(np.float64) - f_0).max() > 1e-5  # the steps did something
    c = case_of(lat, shape, T, S, form)
    c.forced = int(forced)
    c.force = (C.c_double * 3)(*([0.0] * (3 - lat.d) + ([float(x) for x in fv] if forced else [0.0] * lat.d)))
    bufs = [np.ascontiguousarray(f_0.astype(S)), np.zeros_like(f_0, dtype=S)]
    for _ in range(STEPS):
        c.f0, c.f1 = (b.ctypes.data for b in bufs)
        assert emulation.regularized_cpu(LATTICE_ID[lattice], C.byref(c)) == 0
        bufs = [bufs[1], bufs[0]]
    got = bufs[0]
    assert np.array_equal(got, exp), f"{int((got != exp).sum())} of {exp.size} values differ, max {np.abs(got.astype(float) - exp).max():.3e}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("form", ref.FORMS)
@pytest.mark.parametrize("lattice", sorted(SHAPES))
def test_emulated_operator_matches_the_restatement(emulation, lattice, form, dtype):
    """the stand-alone operator: feq is an input field, rho and u are f's moments"""
    lat, shape = orc.Lattice(lattice), SHAPES[lattice]
    policy = "FP32FP32" if dtype is np.float32 else "FP64FP64"
    f = orc.stream(ref.sheared_state(shape, lat, policy).astype(dtype), lat)  # (streamed: off equilibrium)
    rho, u = orc.macroscopic(f, lat)
    feq = orc.equilibrium(rho, u, lat, dtype)
    exp = ref.collide(f, feq, u, OMEGA, lat, form)
    c = case_of(lat, shape, dtype, dtype, form)
    fin, io = np.ascontiguousarray(f), np.ascontiguousarray(feq.copy())
    c.f0, c.f1 = fin.ctypes.data, io.ctypes.data
    assert emulation.regularized_operator_cpu(LATTICE_ID[lattice], C.byref(c)) == 0
    assert np.array_equal(io, exp), f"{int((io != exp).sum())} of {exp.size} values differ, max {np.abs(io.astype(float) - exp).max():.3e}"
