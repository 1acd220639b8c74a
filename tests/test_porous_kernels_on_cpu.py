"""The porous device code without a GPU: xlb_amd/csrc/porous_kernels.hpp is compiled for the host (tests/hip_on_cpu stands in for the
HIP runtime header, -ffp-contract=off as in the library's build), tests/porous_cpu_emulation.cpp runs one forward and one adjoint step
cell by cell with the functions the fused kernels call per cell, and the result is compared with the NumPy restatement
tests/_porous_ref.py BIT FOR BIT: the forward populations, the carried state mu, the cotangent lam, the per-cell omega terms and the
per-cell alpha terms.  This checks the rules and their operation order — not the fused kernels' addressing nor the GPU's code generation,
which tests/test_gpu_porous.py covers."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _adjoint_cases as cases
import _porous_ref as ref
from test_adjoint_kernels_on_cpu import DTYPE_CODE, KIND_CODE, LATTICE_ID, POLICIES, bc_values, differing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OMEGA = 1.3


class Case(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("f_n", "f_out", "lam", "mu", "lam_prev", "alpha", "terms", "galpha", "bc", "miss")] + [
        (n, C.c_int) for n in ("nx", "ny", "nz", "sdt", "cdt")] + [("kind", C.c_void_p), ("values", C.c_void_p), ("omega", C.c_double)]


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    assert cxx, "no clang++ to compile the kernel headers for the host"
    so = tmp_path_factory.mktemp("porous_cpu") / "libporous_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "porous_cpu_emulation.cpp"),
                    "-o", str(so)], check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.porous_cpu.argtypes = [C.c_int, C.POINTER(Case)]
    return lib


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_emulated_porous_steps_match_the_restatement(emulation, name, policy):
    lat, shape, bcs = cases.HOST_CASES[name]()
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    bm, mm = cases.masks(shape, lat, bcs)
    alpha = np.ascontiguousarray(np.random.default_rng(17).uniform(0.0, 0.9, (1,) + shape).astype(T))
    f_n = np.ascontiguousarray(orc.perturbed_init(shape, lat, policy, seed=23, amp_rho=0.02, amp_u=0.03))
    f_n = np.ascontiguousarray(ref.step(f_n, alpha, bm, mm, bcs, OMEGA, lat, policy))  # off equilibrium
    lam = np.ascontiguousarray(np.random.default_rng(9).uniform(-1, 1, f_n.shape).astype(S))
    f_e = ref.step(f_n, alpha, bm, mm, bcs, OMEGA, lat, policy)
    mu_e, terms_e, galpha_e = ref.local_transpose(f_n, lam, alpha, bm, mm, bcs, OMEGA, lat, policy)
    lam_e = ref.adj.stream_transpose(mu_e, bm, mm, bcs, lat, policy)

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
    c.sdt, c.cdt = DTYPE_CODE[np.dtype(S)], DTYPE_CODE[np.dtype(T)]
    c.kind, c.values, c.omega = kind.ctypes.data, values.ctypes.data, OMEGA
    f_out, mu, out = np.zeros_like(f_n), np.zeros_like(f_n), np.zeros_like(f_n)
    terms, galpha = np.zeros(shape, T), np.zeros(shape, T)
    c.f_n, c.f_out, c.lam, c.mu, c.lam_prev = f_n.ctypes.data, f_out.ctypes.data, lam.ctypes.data, mu.ctypes.data, out.ctypes.data
    c.alpha, c.terms, c.galpha = alpha.ctypes.data, terms.ctypes.data, galpha.ctypes.data
    assert emulation.porous_cpu(LATTICE_ID[lat.name], C.byref(c)) == 0
    assert np.array_equal(f_out, f_e), "forward: " + differing(f_out, f_e)
    assert np.array_equal(mu, mu_e), "mu: " + differing(mu, mu_e)
    assert np.array_equal(terms, terms_e), "omega terms: " + differing(terms, terms_e)
    assert np.array_equal(galpha, galpha_e), "alpha terms: " + differing(galpha, galpha_e)
    assert np.array_equal(out, lam_e), "lam: " + differing(out, lam_e)
    assert np.abs(out).max() > 0.1 and np.abs(terms).max() > 0 and np.abs(galpha).max() > 0
