"""The adjoint device code without a GPU: xlb_amd/csrc/adjoint_kernels.hpp is compiled for the host (tests/hip_on_cpu stands in for the
HIP runtime header, -ffp-contract=off as in the library's build), tests/adjoint_cpu_emulation.cpp runs one adjoint step cell by cell
with the functions the fused kernel calls per cell, and the result is compared with the NumPy restatement tests/_adjoint_ref.py BIT
FOR BIT: the carried state mu, the cotangent lam and the per-cell omega terms.  This checks the transposed rules and their operation
order — not the fused kernel's addressing nor the GPU's code generation, which tests/test_gpu_adjoint.py covers."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _adjoint_cases as cases
import _adjoint_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE_ID = {"D2Q9": 0, "D3Q19": 1, "D3Q27": 2}
DTYPE_CODE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}  # XLBHIP_F64, XLBHIP_F32
KIND_CODE = {orc.KIND_EQUILIBRIUM: 1, orc.KIND_HALFWAY_BB: 2, orc.KIND_FULLWAY_BB: 3, orc.KIND_DO_NOTHING: 4}
OMEGA = 1.3
POLICIES = ["FP32FP32", "FP64FP64", "FP64FP32"]


class Case(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("f_n", "lam", "mu", "lam_prev", "terms", "rho_bar", "u_bar", "bc", "miss")] + [
        (n, C.c_int) for n in ("nx", "ny", "nz", "sdt", "cdt")] + [("kind", C.c_void_p), ("values", C.c_void_p), ("omega", C.c_double)]


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("adjoint_cpu") / "libadjoint_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "adjoint_cpu_emulation.cpp"),
                    "-o", str(so)], check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.adjoint_cpu.argtypes = [C.c_int, C.c_int, C.POINTER(Case)]
    return lib


def bc_values(bc, lat, policy):
    """the 27 constants of a BC descriptor, as xlb_amd's boundary conditions compute them (boundary_condition.py: _hip_values)"""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    v = np.zeros(27)
    if bc.kind == orc.KIND_EQUILIBRIUM:
        v[: lat.q] = orc.equilibrium(np.array([bc.rho], T), np.array(bc.u, T), lat, T)
    elif bc.kind == orc.KIND_HALFWAY_BB and bc.u_wall is not None:
        uw = np.asarray(bc.u_wall, dtype=np.float64).astype(S)
        w = lat.w.astype(T)
        for l in range(lat.q):
            dot = S(0)
            for d in range(lat.d):
                dot = S(dot + S(int(lat.c[d, l])) * uw[d])
            v[l] = T(6.0) * (w[l] * T(dot))
    return v


def base_case(lat, policy, shape, bm, mm, bcs):
    kind, values = np.zeros(256, np.uint8), np.zeros((256, 27))
    for bc in bcs:
        kind[bc.id] = KIND_CODE[bc.kind]
        values[bc.id] = bc_values(bc, lat, policy)
    bits = np.zeros(shape, np.uint32)
    for l in range(lat.q):
        bits |= mm[l].astype(np.uint32) << np.uint32(l)
    bcm = np.ascontiguousarray(bm[0])
    c = Case()
    c.bc, c.miss = bcm.ctypes.data, bits.ctypes.data
    c.nx, c.ny, c.nz = (1,) * (3 - lat.d) + tuple(shape)
    c.sdt, c.cdt = DTYPE_CODE[np.dtype(orc.store_dtype(policy))], DTYPE_CODE[np.dtype(orc.compute_dtype(policy))]
    c.kind, c.values, c.omega = kind.ctypes.data, values.ctypes.data, OMEGA
    return c, (kind, values, bits, bcm)


def differing(a, b):
    return f"{int((a != b).sum())} of {b.size} values differ, max {np.abs(a.astype(float) - b).max():.3e}"


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_emulated_adjoint_step_matches_the_restatement(emulation, name, policy):
    lat, shape, bcs = cases.HOST_CASES[name]()
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    bm, mm = cases.masks(shape, lat, bcs)
    f_n = np.ascontiguousarray(orc.perturbed_init(shape, lat, policy, seed=23, amp_rho=0.02, amp_u=0.03))
    f_n = np.ascontiguousarray(orc.step(f_n, bm, mm, bcs, OMEGA, lat, policy))  # off equilibrium
    lam = np.ascontiguousarray(np.random.default_rng(9).uniform(-1, 1, f_n.shape).astype(S))
    mu_e, terms_e = ref.local_transpose(f_n, lam, bm, mm, bcs, OMEGA, lat, policy)
    lam_e = ref.stream_transpose(mu_e, bm, mm, bcs, lat, policy)
    c, keep = base_case(lat, policy, shape, bm, mm, bcs)
    mu, out, terms = np.zeros_like(f_n), np.zeros_like(f_n), np.zeros(shape, T)
    c.f_n, c.lam, c.mu, c.lam_prev, c.terms = f_n.ctypes.data, lam.ctypes.data, mu.ctypes.data, out.ctypes.data, terms.ctypes.data
    assert emulation.adjoint_cpu(LATTICE_ID[lat.name], 0, C.byref(c)) == 0
    assert np.array_equal(mu, mu_e), "mu: " + differing(mu, mu_e)
    assert np.array_equal(terms, terms_e), "omega terms: " + differing(terms, terms_e)
    assert np.array_equal(out, lam_e), "lam: " + differing(out, lam_e)
    assert np.abs(out).max() > 0.1 and np.abs(terms).max() > 0


@pytest.mark.parametrize("lattice,policy,shape", [("D3Q19", "FP32FP32", (5, 6, 4)), ("D3Q27", "FP64FP32", (3, 4, 5)), ("D2Q9", "FP64FP64", (6, 5))])
def test_emulated_macroscopic_adjoint_kernel(emulation, lattice, policy, shape):
    lat = orc.Lattice(lattice)
    T = orc.compute_dtype(policy)
    f = np.ascontiguousarray(orc.perturbed_init(shape, lat, policy, seed=3, amp_rho=0.02, amp_u=0.03))
    rng = np.random.default_rng(4)
    rho_bar = np.ascontiguousarray(rng.uniform(-1, 1, (1,) + shape).astype(T))
    u_bar = np.ascontiguousarray(rng.uniform(-1, 1, (lat.d,) + shape).astype(T))
    c, keep = base_case(lat, policy, shape, np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool), [])
    out = np.zeros_like(f)
    c.f_n, c.rho_bar, c.u_bar, c.lam_prev = f.ctypes.data, rho_bar.ctypes.data, u_bar.ctypes.data, out.ctypes.data
    assert emulation.adjoint_cpu(LATTICE_ID[lattice], 1, C.byref(c)) == 0
    exp = ref.macroscopic_adjoint(f, rho_bar, u_bar, lat, policy)
    assert np.array_equal(out, exp), differing(out, exp)
