"""The two-component Shan-Chen device code without a GPU: xlb_amd/csrc/multicomponent_kernels.hpp is compiled for the host
(tests/hip_on_cpu stands in for the HIP runtime header, -ffp-contract=off as in the library's build),
tests/multicomponent_cpu_emulation.cpp runs steps cell by cell with the functions the row kernels call per cell, and both population sets,
the densities, both forces and the physical velocity are compared with the NumPy restatement tests/_multicomponent_ref.py BIT FOR BIT, on
the set-ups of the device test in all three policies.  Not covered: the row kernels' addressing and the GPU's code generation
(tests/test_gpu_multicomponent.py).

Which of these tests see a wrong scheme (neither mutation is committed; profiles/multicomponent.md has the table): with S^A and S^B
swapped in F^A, and with omega dropped from the weights of u', all 24 cases fail."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _multicomponent_cases as cases
import _multicomponent_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICE_ID = {"D2Q9": 0, "D3Q19": 1, "D3Q27": 2}
DTYPE_CODE = {np.dtype(np.float64): 0, np.dtype(np.float32): 1}  # XLBHIP_F64, XLBHIP_F32
KIND_CODE = {orc.KIND_HALFWAY_BB: 2, orc.KIND_FULLWAY_BB: 3}
OUTPUTS = ("psi_a", "psi_b", "rho_a", "rho_b", "u", "force_a", "force_b")


class Case(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("fa0", "fa1", "fb0", "fb1") + OUTPUTS + ("bc", "miss")] + [(n, C.c_int) for n in ("nx", "ny", "nz", "sdt", "cdt")]
                + [(n, C.c_void_p) for n in ("kind", "wall_a", "wall_b")] + [(n, C.c_double) for n in ("g_aa", "g_ab", "g_bb")] + [("fvec", C.c_double * 3)]
                + [(n, C.c_double) for n in ("omega_a", "omega_b")])


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("multicomponent_cpu") / "libmulticomponent_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "multicomponent_cpu_emulation.cpp"), "-o", str(so)], check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.multicomponent_cpu.argtypes = [C.c_int, C.POINTER(Case)]
    return lib


def run_emulated(lib, lattice, policy, fa_0, fb_0, bm, mm, bcs, wall_density, steps, force_vector):
    lat = orc.Lattice(lattice)
    T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
    shape = fa_0.shape[1:]
    kind = np.zeros(256, np.uint8)
    for bc in bcs:
        assert bc.u_wall is None
        kind[bc.id] = KIND_CODE[bc.kind]
    wall_a, wall_b = (t.astype(np.float64) for t in ref.wall_tables(wall_density, T))
    bits = np.zeros(shape, np.uint32)
    for l in range(lat.q):
        bits |= mm[l].astype(np.uint32) << np.uint32(l)
    bcm = np.ascontiguousarray(bm[0])
    a = [np.ascontiguousarray(fa_0.astype(S)), np.zeros_like(fa_0, dtype=S)]
    b = [np.ascontiguousarray(fb_0.astype(S)), np.zeros_like(fb_0, dtype=S)]
    out = {k: np.zeros(((lat.d if k in ("u", "force_a", "force_b") else 1),) + shape, T) for k in OUTPUTS}
    c = Case()
    c.bc, c.miss = bcm.ctypes.data, bits.ctypes.data
    c.nx, c.ny, c.nz = (1,) * (3 - lat.d) + shape
    c.sdt, c.cdt = DTYPE_CODE[np.dtype(S)], DTYPE_CODE[np.dtype(T)]
    c.kind, c.wall_a, c.wall_b = kind.ctypes.data, wall_a.ctypes.data, wall_b.ctypes.data
    for k in OUTPUTS:
        setattr(c, k, out[k].ctypes.data)
    c.g_aa, c.g_ab, c.g_bb = cases.G_AA, cases.G_AB, cases.G_BB
    c.omega_a, c.omega_b = cases.OMEGA
    c.fvec = (C.c_double * 3)(*([0.0] * (3 - lat.d) + [float(x) for x in force_vector]))
    for _ in range(steps):
        c.fa0, c.fa1, c.fb0, c.fb1 = a[0].ctypes.data, a[1].ctypes.data, b[0].ctypes.data, b[1].ctypes.data
        assert lib.multicomponent_cpu(LATTICE_ID[lattice], C.byref(c)) == 0
        a, b = a[::-1], b[::-1]
    return a[0], b[0], out  # out: of the LAST step's start state


# the set-ups of tests/test_gpu_multicomponent.py
SETUPS = [
    ("periodic", cases.periodic, "D3Q19", (5, 6, 7)),
    ("periodic", cases.periodic, "D3Q19", (2, 3, 4)),
    ("periodic", cases.periodic, "D3Q27", (4, 5, 6)),
    ("periodic", cases.periodic, "D2Q9", (7, 9)),
    ("long-walls", cases.long_walls, "D2Q9", (3, 320)),
    ("halfway-box", cases.halfway_box, "D3Q19", (6, 6, 6)),
    ("fullway-box", cases.fullway_box, "D3Q19", (6, 6, 6)),
    ("solid-block", cases.solid_block, "D3Q19", (8, 8, 8)),
]


@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP64", "FP64FP32"])
@pytest.mark.parametrize("name,build,lattice,shape", SETUPS, ids=[f"{c[0]}-{c[2]}-{'x'.join(map(str, c[3]))}" for c in SETUPS])
def test_emulated_steps_match_the_restatement(emulation, name, build, lattice, shape, policy):
    lat = orc.Lattice(lattice)
    setup = build(shape, cases.WALL_LO, cases.WALL_HI)
    bcs, wall_density = setup.oracle()
    bm, mm = setup.masks(shape, lat, bcs)
    fa_0, fb_0 = cases.random_states(shape, lat, policy, seed=17)
    mix = cases.mixture()
    fv = cases.force_vector(lat)
    steps = 3
    kw = dict(wall_density=wall_density, policy=policy, force_vector=fv)
    fa_b, fb_b = ref.run(fa_0, fb_0, bm, mm, bcs, cases.OMEGA, lat, mix, steps - 1, **kw)
    parts = {}
    fa_e, fb_e = ref.step(fa_b, fb_b, bm, mm, bcs, cases.OMEGA, lat, mix, parts=parts, **kw)
    assert np.isfinite(fa_e).all() and np.isfinite(fb_e).all()
    assert min(np.abs(parts["force_a"]).max(), np.abs(parts["force_b"]).max()) > 1e-4  # the interaction matters in the case
    if bcs:  # ... and so do the walls: some neighbour was replaced by a wall value
        assert any(((bm[0] != 0) & mm[lat.opp[i]]).any() for i in range(1, lat.q))
    fa_k, fb_k, out = run_emulated(emulation, lattice, policy, fa_0, fb_0, bm, mm, bcs, wall_density, steps, fv)
    for key, exp in (("psi_a", parts["psi_a"]), ("psi_b", parts["psi_b"]), ("rho_a", parts["rho_a"]), ("rho_b", parts["rho_b"]), ("force_a", parts["force_a"]),
                     ("force_b", parts["force_b"]), ("u", parts["u_phys"])):
        assert np.array_equal(out[key], exp), f"{key}: {int((out[key] != exp).sum())} of {exp.size} values differ, max {np.abs(out[key].astype(float) - exp).max():.3e}"
    for key, got, exp in (("f_A", fa_k, fa_e), ("f_B", fb_k, fb_e)):
        assert np.array_equal(got, exp), f"{key}: {int((got != exp).sum())} of {exp.size} values differ, max {np.abs(got.astype(float) - exp).max():.3e}"
