"""The Shan-Chen device code without a GPU: xlb_amd/csrc/multiphase_kernels.hpp is compiled for the host (tests/hip_on_cpu stands in for
the HIP runtime header, -ffp-contract=off as in the library's build), tests/multiphase_cpu_emulation.cpp runs steps cell by cell with the
functions the row kernels call per cell, and populations, psi, force, rho and physical velocity are compared with the NumPy restatement
tests/_multiphase_ref.py BIT FOR BIT.  ShanChenDensity and CarnahanStarling only (the exponential form's exp is the C library's here and
ocml's on the device; neither is NumPy's).  Not covered: the row kernels' addressing and the GPU's code generation
(tests/test_gpu_multiphase.py)."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _multiphase_cases as cases
import _multiphase_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE_ID = {"D2Q9": 0, "D3Q19": 1, "D3Q27": 2}
DTYPE_CODE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}  # XLBHIP_F64, XLBHIP_F32
KIND_CODE = {orc.KIND_HALFWAY_BB: 2, orc.KIND_FULLWAY_BB: 3}
OMEGA = 1.2
T_CS = 0.8 * ref.CarnahanStarling.critical_temperature()


class Case(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("f0", "f1", "psi", "rho", "u", "force", "bc", "miss")] + [(n, C.c_int) for n in ("nx", "ny", "nz", "sdt", "cdt")] + [
        (n, C.c_void_p) for n in ("kind", "values", "psi_wall")] + [("form", C.c_int), ("g", C.c_double), ("par", C.c_double * 4), ("fvec", C.c_double * 3),
                                                                     ("omega", C.c_double)]


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("multiphase_cpu") / "libmultiphase_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "multiphase_cpu_emulation.cpp"),
                    "-o", str(so)], check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.multiphase_cpu.argtypes = [C.c_int, C.POINTER(Case)]
    return lib


def halfway_values(bc, lat, policy):
    """the moving-wall constants of a halfway wall's descriptor, as HalfwayBounceBackBC._hip_values computes them"""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    v = np.zeros(27)
    if bc.kind == orc.KIND_HALFWAY_BB and bc.u_wall is not None:
        uw = np.asarray(bc.u_wall, dtype=np.float64).astype(S)
        w = lat.w.astype(T)
        for l in range(lat.q):
            dot = S(0)
            for d in range(lat.d):
                dot = S(dot + S(int(lat.c[d, l])) * uw[d])
            v[l] = T(6.0) * (w[l] * T(dot))
    return v


def model_of(form):
    """(restatement model, form id, parameters)"""
    if form == "density":
        return ref.Density(-0.6), 1, []
    return ref.CarnahanStarling(T_CS), 2, [T_CS, 1.0, 4.0, 1.0]


def run_emulated(lib, lattice, policy, f_0, bm, mm, bcs, form, wall_density, steps, force_vector=None):
    lat = orc.Lattice(lattice)
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    model, form_id, par = model_of(form)
    shape = f_0.shape[1:]
    kind, values = np.zeros(256, np.uint8), np.zeros((256, 27))
    for bc in bcs:
        kind[bc.id] = KIND_CODE[bc.kind]
        values[bc.id] = halfway_values(bc, lat, policy)
    psi_wall = ref.wall_table(model, wall_density, T).astype(np.float64)
    bits = np.zeros(shape, np.uint32)
    for l in range(lat.q):
        bits |= mm[l].astype(np.uint32) << np.uint32(l)
    bcm = np.ascontiguousarray(bm[0])
    bufs = [np.ascontiguousarray(f_0.astype(S)), np.zeros_like(f_0, dtype=S)]
    out = {"psi": np.zeros((1,) + shape, T), "rho": np.zeros((1,) + shape, T), "u": np.zeros((lat.d,) + shape, T), "force": np.zeros((lat.d,) + shape, T)}
    c = Case()
    c.bc, c.miss = bcm.ctypes.data, bits.ctypes.data
    c.nx, c.ny, c.nz = (1,) * (3 - lat.d) + shape
    c.sdt, c.cdt = DTYPE_CODE[np.dtype(S)], DTYPE_CODE[np.dtype(T)]
    c.kind, c.values, c.psi_wall = kind.ctypes.data, values.ctypes.data, psi_wall.ctypes.data
    c.psi, c.rho, c.u, c.force = (out[k].ctypes.data for k in ("psi", "rho", "u", "force"))
    c.form, c.g, c.omega = form_id, model.G, OMEGA
    c.par = (C.c_double * 4)(*(par + [0.0] * (4 - len(par))))
    c.fvec = (C.c_double * 3)(*([0.0] * (3 - lat.d) + [float(x) for x in (force_vector if force_vector is not None else [0.0] * lat.d)]))
    for _ in range(steps):
        c.f0, c.f1 = (b.ctypes.data for b in bufs)
        assert lib.multiphase_cpu(LATTICE_ID[lattice], C.byref(c)) == 0
        bufs = [bufs[1], bufs[0]]
    return bufs[0], out  # out: of the LAST step's start state


# (name, set-up, lattice, policy, shape, form, force vector)
CASES = [
    ("periodic", cases.periodic, "D3Q19", "FP32FP32", (5, 6, 4), "density", False),
    ("periodic", cases.periodic, "D2Q9", "FP64FP64", (5, 7), "cs", True),
    ("periodic", cases.periodic, "D3Q27", "FP64FP32", (4, 5, 3), "cs", False),
    ("periodic", cases.periodic, "D3Q19", "FP32FP32", (2, 3, 4), "cs", False),
    ("halfway-box", cases.halfway_box, "D3Q19", "FP32FP32", (6, 6, 6), "density", True),
    ("halfway-box", cases.halfway_box, "D3Q19", "FP64FP64", (6, 6, 6), "cs", False),
    ("halfway-box", cases.halfway_box, "D2Q9", "FP64FP64", (7, 8), "cs", False),
    ("plates", cases.halfway_plates, "D2Q9", "FP32FP32", (5, 9), "density", True),
    ("fullway-box", cases.fullway_box, "D3Q19", "FP32FP32", (6, 6, 6), "cs", False),
    ("fullway-box", cases.fullway_box, "D3Q27", "FP64FP32", (5, 6, 5), "density", True),
    ("solid-block", cases.solid_block, "D3Q19", "FP64FP64", (8, 8, 8), "cs", False),
    ("solid-block", cases.solid_block, "D3Q27", "FP32FP32", (7, 8, 6), "density", False),
]
DENSITY_RANGE = {"density": (0.8, 1.2, 0.7, 1.1), "cs": (0.08, 0.3, 0.05, 0.25)}  # start state lo, hi; the two wall densities


@pytest.mark.parametrize("name,build,lattice,policy,shape,form,forced", CASES, ids=[f"{c[0]}-{c[2]}-{c[3]}-{c[5]}{'-forced' if c[6] else ''}" for c in CASES])
def test_emulated_steps_match_the_restatement(emulation, name, build, lattice, policy, shape, form, forced):
    lat = orc.Lattice(lattice)
    lo, hi, w_lo, w_hi = DENSITY_RANGE[form]
    setup = build(shape, w_lo, w_hi)
    bcs, wall_density = setup.oracle()
    bm, mm = setup.masks(shape, lat, bcs)
    f_0 = cases.random_state(shape, lat, policy, lo, hi, seed=17)
    model, _, _ = model_of(form)
    fv = np.array([1e-4, -2e-4, 3e-4])[: lat.d] if forced else None
    steps = 3
    kw = dict(wall_density=wall_density, policy=policy, force_vector=fv)
    f_before = ref.run(f_0, bm, mm, bcs, OMEGA, lat, model, steps - 1, **kw)
    parts = {}
    f_e = ref.step(f_before, bm, mm, bcs, OMEGA, lat, model, parts=parts, **kw)
    assert np.isfinite(f_e).all() and np.isfinite(parts["psi"]).all()
    assert np.abs(parts["force"]).max() > 1e-4  # the interaction matters in the case
    if bcs:  # ... and so do the walls: some neighbour was replaced by a wall value
        ids = bm[0]
        assert any(((ids != 0) & mm[lat.opp[i]]).any() for i in range(1, lat.q))
    f_k, out = run_emulated(emulation, lattice, policy, f_0, bm, mm, bcs, form, wall_density, steps, force_vector=fv)
    for key, exp in (("psi", parts["psi"]), ("rho", parts["rho"]), ("force", parts["force"]), ("u", parts["u_phys"])):
        assert np.array_equal(out[key], exp), f"{key}: {int((out[key] != exp).sum())} of {exp.size} values differ, max {np.abs(out[key].astype(float) - exp).max():.3e}"
    assert np.array_equal(f_k, f_e), f"f: {int((f_k != f_e).sum())} of {f_e.size} values differ, max {np.abs(f_k.astype(float) - f_e).max():.3e}"
