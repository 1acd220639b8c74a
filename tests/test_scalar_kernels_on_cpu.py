"""The scalar-transport device code without a GPU: xlb_amd/csrc/scalar_kernels.hpp is compiled for the host (tests/hip_on_cpu stands in
for the HIP runtime header, -ffp-contract=off as in the library's build), tests/scalar_cpu_emulation.cpp runs one coupled step cell by
cell with the functions the fused kernel calls per cell, and the result is compared with the NumPy restatement tests/_scalar_ref.py
BIT FOR BIT.  This checks the scalar rules, the direction table, the collision, the per-cell force and the two small kernels — not the
fused kernel's addressing nor the GPU's code generation, which tests/test_gpu_scalar_transport.py covers.  BGK only: the fp64 KBC
collision of cell.hpp pins registers with GPU inline assembly."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _scalar_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE_ID = {"D2Q9": 0, "D3Q19": 1, "D3Q27": 2}
DTYPE_CODE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}  # XLBHIP_F64, XLBHIP_F32
KIND_CODE = {orc.KIND_EQUILIBRIUM: 1, orc.KIND_HALFWAY_BB: 2, orc.KIND_FULLWAY_BB: 3, orc.KIND_DO_NOTHING: 4, orc.KIND_REGULARIZED_VELOCITY: 7,
             orc.KIND_EXTRAPOLATION_OUTFLOW: 9}
RULE_CODE = {ref.ADIABATIC: 0, ref.DIRICHLET: 1, ref.DO_NOTHING: 2}
OMEGA, OMEGA_S = 1.3, 1.45


class Coupling(C.Structure):
    _fields_ = [("force", C.c_double * 3), ("buoyancy", C.c_double * 3), ("reference", C.c_double)]


class Case(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("f0", "f1", "g0", "g1", "phi", "bc", "miss")] + [(n, C.c_int) for n in ("nx", "ny", "nz", "sdt", "cdt", "forced")] + [
        (n, C.c_void_p) for n in ("kind", "values", "rule", "rvalue")] + [("omega", C.c_double), ("omega_s", C.c_double), ("cp", Coupling)]


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("scalar_cpu") / "libscalar_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "scalar_cpu_emulation.cpp"),
                    "-o", str(so)], check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.scalar_cpu.argtypes = [C.c_int, C.c_int, C.c_double, C.POINTER(Case)]
    return lib


def bc_values(bc, lat, policy):
    """the 27 constants of a BC descriptor, as xlb_amd's boundary conditions compute them (boundary_condition.py: _hip_values)"""
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    v = np.zeros(27)
    if bc.kind == orc.KIND_EQUILIBRIUM:
        v[: lat.q] = orc.equilibrium(np.array([bc.rho], T), np.array(bc.u, T), lat, T)
    elif bc.kind == orc.KIND_REGULARIZED_VELOCITY:
        v[3 - lat.d : 3] = np.asarray(bc.prescribed, np.float64).astype(S)
    elif bc.kind == orc.KIND_EXTRAPOLATION_OUTFLOW:
        cs = T(1.0) / np.sqrt(T(3.0))
        v[3 - lat.d : 3] = bc.normal
        v[3], v[4] = cs, T(1.0) - cs
    return v


def run_emulated(lib, lattice, policy, f_0, g_0, bm, mm, bcs, rules, steps, force_vector=None, buoyancy=None, reference=0.0):
    lat = orc.Lattice(lattice)
    S = orc.store_dtype(policy)
    shape3 = (1,) * (3 - lat.d) + f_0.shape[1:]
    kind, values = np.zeros(256, np.uint8), np.zeros((256, 27))
    for bc in bcs:
        kind[bc.id] = KIND_CODE[bc.kind]
        values[bc.id] = bc_values(bc, lat, policy)
    rule, rvalue = np.zeros(256, np.uint8), np.zeros(256)
    for r in rules:
        rule[r.id], rvalue[r.id] = RULE_CODE[r.kind], r.value
    bits = np.zeros(f_0.shape[1:], np.uint32)
    for l in range(lat.q):
        bits |= mm[l].astype(np.uint32) << np.uint32(l)
    bcm = np.ascontiguousarray(bm[0])
    bufs = [np.ascontiguousarray(f_0.astype(S)), np.zeros_like(f_0, dtype=S), np.ascontiguousarray(g_0.astype(S)), np.zeros_like(g_0, dtype=S)]
    c = Case()
    c.bc, c.miss = bcm.ctypes.data, bits.ctypes.data
    c.nx, c.ny, c.nz = shape3
    c.sdt, c.cdt = DTYPE_CODE[np.dtype(S)], DTYPE_CODE[np.dtype(orc.compute_dtype(policy))]
    c.forced = int(force_vector is not None or buoyancy is not None)
    c.kind, c.values, c.rule, c.rvalue = kind.ctypes.data, values.ctypes.data, rule.ctypes.data, rvalue.ctypes.data
    c.omega, c.omega_s = OMEGA, OMEGA_S
    pad = lambda v: [0.0] * (3 - lat.d) + [float(x) for x in (v if v is not None else [0.0] * lat.d)]  # noqa: E731
    c.cp = Coupling((C.c_double * 3)(*pad(force_vector)), (C.c_double * 3)(*pad(buoyancy)), reference)
    for _ in range(steps):
        c.f0, c.f1, c.g0, c.g1 = (b.ctypes.data for b in bufs)
        assert lib.scalar_cpu(LATTICE_ID[lattice], 0, 0.0, C.byref(c)) == 0
        bufs = [bufs[1], bufs[0], bufs[3], bufs[2]]
    return bufs[0], bufs[2]


# ---- the cases: oracle BCs + restatement rules -------------------------------------------------------------------------------------------
def faces(shape, remove_edges=False):
    return orc.bounding_box_indices(shape, remove_edges=remove_edges)


def union(*index_lists):
    return np.unique(np.concatenate([np.asarray(i) for i in index_lists], axis=1), axis=-1).tolist()


def periodic(shape):
    return [], []


def heated_box(shape):
    d = len(shape)
    f, f_ne = faces(shape), faces(shape, remove_edges=True)
    sides = union(*[f[s] for s in (["left", "right"] + (["front", "back"] if d == 3 else []))])
    bcs = [orc.BC(orc.KIND_EQUILIBRIUM, 1, f_ne["top"], rho=1.0, u=(0.02, 0.0, 0.0)[:d]), orc.BC(orc.KIND_HALFWAY_BB, 2, f_ne["bottom"]),
           orc.BC(orc.KIND_HALFWAY_BB, 3, sides)]
    return bcs, [ref.Rule(ref.DIRICHLET, 2, 1.0), ref.Rule(ref.DIRICHLET, 1, 0.0)]


def channel(shape):
    f, f_ne = faces(shape), faces(shape, remove_edges=True)
    sides = union(*[f[s] for s in ("bottom", "top", "front", "back")])
    bcs = [orc.BC(orc.KIND_FULLWAY_BB, 1, sides), orc.BC(orc.KIND_REGULARIZED_VELOCITY, 2, f_ne["left"], prescribed=(0.03, 0.0, 0.0)),
           orc.BC(orc.KIND_EXTRAPOLATION_OUTFLOW, 3, f_ne["right"])]
    return bcs, [ref.Rule(ref.DIRICHLET, 2, 1.25), ref.Rule(ref.DO_NOTHING, 3), ref.Rule(ref.ADIABATIC, 1)]


def heated_sphere(shape):
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    inside = (x - shape[0] // 2) ** 2 + (y - shape[1] // 2) ** 2 + (z - shape[2] // 2) ** 2 < 1.6**2
    return [orc.BC(orc.KIND_HALFWAY_BB, 1, [a.tolist() for a in np.nonzero(inside)])], [ref.Rule(ref.DIRICHLET, 1, 1.5)]


CASES = [
    ("periodic", periodic, "D3Q19", "FP32FP32", (5, 6, 4), False),
    ("periodic", periodic, "D2Q9", "FP64FP64", (5, 7), True),
    ("box", heated_box, "D3Q19", "FP32FP32", (7, 6, 6), False),
    ("box", heated_box, "D3Q19", "FP64FP64", (7, 6, 6), True),
    ("box", heated_box, "D2Q9", "FP64FP64", (7, 8), True),
    ("channel", channel, "D3Q19", "FP32FP32", (9, 6, 7), False),
    ("channel", channel, "D3Q27", "FP64FP32", (9, 6, 7), False),
    ("sphere", heated_sphere, "D3Q27", "FP64FP32", (8, 7, 8), True),
    ("sphere", heated_sphere, "D3Q19", "FP32FP32", (8, 7, 8), False),
]


@pytest.mark.parametrize("name,build,lattice,policy,shape,buoyant", CASES, ids=[f"{c[0]}-{c[2]}-{c[3]}{'-buoyant' if c[5] else ''}" for c in CASES])
def test_emulated_step_matches_the_restatement(emulation, name, build, lattice, policy, shape, buoyant):
    lat = orc.Lattice(lattice)
    bcs, rules = build(shape)
    bm, mm = orc.build_masks(shape, lat, bcs) if bcs else (np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool))
    f_0 = orc.perturbed_init(shape, lat, policy, seed=23, amp_rho=0.02, amp_u=0.03)
    g_0 = ref.init_g(np.random.default_rng(7).uniform(0.5, 1.5, shape), f_0, lat, policy)
    coupling = dict(force_vector=np.array([1e-5, 0.0, 0.0])[: lat.d], buoyancy=np.array([0.0, 0.0, 2e-2])[-lat.d :], reference=0.5) if buoyant else {}
    steps = 4
    acted = {}
    with np.errstate(all="ignore"):
        f_e, g_e = ref.run(f_0, g_0, bm, mm, bcs, rules, OMEGA, OMEGA_S, lat, steps, policy=policy, acted=acted, **coupling)
    assert all(acted.get(r.id, 0) > 0 for r in rules)
    f_k, g_k = run_emulated(emulation, lattice, policy, f_0, g_0, bm, mm, bcs, rules, steps, **coupling)
    assert np.array_equal(g_k, g_e), f"g: {int((g_k != g_e).sum())} of {g_e.size} values differ, max {np.abs(g_k.astype(float) - g_e).max():.3e}"
    assert np.array_equal(f_k, f_e), f"f: {int((f_k != f_e).sum())} of {f_e.size} values differ, max {np.abs(f_k.astype(float) - f_e).max():.3e}"


@pytest.mark.parametrize("lattice,policy,shape", [("D3Q19", "FP32FP32", (5, 6, 4)), ("D3Q27", "FP64FP32", (3, 4, 5)), ("D2Q9", "FP64FP64", (6, 5))])
def test_emulated_init_and_moment_kernels(emulation, lattice, policy, shape):
    lat = orc.Lattice(lattice)
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    f_0 = np.ascontiguousarray(orc.perturbed_init(shape, lat, policy, seed=3, amp_rho=0.02, amp_u=0.03))
    phi0 = np.ascontiguousarray(np.random.default_rng(4).uniform(0.5, 1.5, shape).astype(T))
    c = Case()
    c.nx, c.ny, c.nz = (1,) * (3 - lat.d) + shape
    c.sdt, c.cdt = DTYPE_CODE[np.dtype(S)], DTYPE_CODE[np.dtype(T)]
    for phi, const in ((phi0, 0.0), (None, 0.75)):
        g = np.zeros((2 * lat.d + 1,) + shape, S)
        c.f0, c.g0, c.phi = f_0.ctypes.data, g.ctypes.data, None if phi is None else phi.ctypes.data
        assert emulation.scalar_cpu(LATTICE_ID[lattice], 1, const, C.byref(c)) == 0
        assert np.array_equal(g, ref.init_g(const if phi is None else phi, f_0, lat, policy))
    out = np.zeros(shape, T)
    c.phi = out.ctypes.data
    assert emulation.scalar_cpu(LATTICE_ID[lattice], 2, 0.0, C.byref(c)) == 0
    assert np.array_equal(out, ref.moment(g, policy)[0]) and np.abs(out - 0.75).max() < 1e-6
