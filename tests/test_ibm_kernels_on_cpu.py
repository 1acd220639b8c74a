"""The coupling kernels of the immersed-boundary stepper without a GPU: xlb_amd/csrc/ibm_kernels.hpp is compiled for the host
(tests/hip_on_cpu stands in for the HIP runtime header, tests/ibm_cpu_emulation.cpp launches the kernels in the order of csrc/ibm.hip
with one emulated thread after the other) and compared with the NumPy restatement, tests/_ibm_ref.py, at the tolerance of the GPU tests
(1e-6 absolute on rho, u and the forces).  This checks the kernels' arithmetic, indexing, fixed-point accumulation and early exit —
not the GPU's code generation nor concurrent atomics, which tests/test_gpu_ibm.py covers."""

import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import xlb_numpy as orc

import _ibm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (24, 24, 24)
TOL = 1e-6


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    # (_Float16 in the kernel headers: clang, e.g. the one the ROCm toolchain ships)
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("ibm_cpu") / "libibm_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "ibm_cpu_emulation.cpp"),
                    "-o", str(so)], check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.couple_cpu.argtypes = ([C.c_int, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_int64] + [C.c_void_p] * 3
                               + [C.c_int, C.c_double, C.c_double, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)])

    def couple(lattice, policy, f_1, pos, areas, vel, sweeps=4, tolerance=1e-5, relaxation=0.5):
        T, S = orc.compute_dtype(policy), orc.store_dtype(policy)
        f = np.ascontiguousarray(f_1.astype(S)).copy()
        pos, areas, vel = (np.ascontiguousarray(a, np.float32) for a in (pos, areas, vel))
        F, used, cells = np.zeros((len(pos), 3)), C.c_int(), C.c_int64()
        rc = lib.couple_cpu({"D3Q19": 1, "D3Q27": 2}[lattice], int(T == np.float32), int(S == np.float32), f.ctypes.data, *f.shape[1:], len(pos),
                            pos.ctypes.data, areas.ctypes.data, vel.ctypes.data, sweeps, tolerance, relaxation, F.ctypes.data, C.byref(used), C.byref(cells))
        assert rc == 0, "k_ibm_clear left cells in the map"
        return f, F, used.value, cells.value

    return couple


def body(centre=(11.3, 12.6, 11.85), n=400, radius=5.3):
    pos = ref.fibonacci_sphere(n, radius, centre)
    areas = np.full(n, 4 * np.pi * radius**2 / n, dtype=np.float32)
    vel = np.tile(np.array([0.02, 0.01, -0.005], dtype=np.float32), (n, 1))
    return pos, areas, vel


@pytest.mark.parametrize("lattice,collision,policy", [("D3Q19", "BGK", "FP32FP32"), ("D3Q27", "KBC", "FP64FP64"), ("D3Q19", "BGK", "FP64FP32")])
def test_kernels_match_the_restatement(emulation, lattice, collision, policy):
    lat = orc.Lattice(lattice)
    T = orc.compute_dtype(policy)
    pos, areas, vel = body()
    bm, mm = np.zeros((1,) + SHAPE, np.uint8), np.zeros((lat.q,) + SHAPE, bool)
    f_e = f_k = orc.perturbed_init(SHAPE, lat, policy, seed=7)
    for _ in range(4):
        with np.errstate(all="ignore"):
            s_e = orc.step(f_e, bm, mm, [], 1.2, lat, policy, collision)
            s_k = orc.step(f_k, bm, mm, [], 1.2, lat, policy, collision)
        exp = ref.couple(s_e, pos, areas, vel, lat, policy, relaxation=0.5)
        f_k, F, used, cells = emulation(lattice, policy, s_k, pos, areas, vel)
        f_e = exp["f"]
        outside = exp["W"] == 0
        assert used == exp["sweeps"] == 4 and cells == int((~outside).sum())
        assert np.array_equal(f_k[:, outside], s_k[:, outside])  # nothing outside the footprint
    rho, u = orc.macroscopic(f_k.astype(T), lat)
    rho_e, u_e = orc.macroscopic(f_e.astype(T), lat)
    figures = (np.abs(rho.astype(float) - rho_e).max(), np.abs(u.astype(float) - u_e).max(), np.abs(F - exp["forces"]).max())
    print(lattice, collision, policy, "max |d rho| %.2e  |d u| %.2e  |d F| %.2e" % figures)
    assert max(figures) <= TOL, figures
    assert np.abs(exp["G"]).max() > 1e-3


def test_early_exit_and_marker_order(emulation):
    lat = orc.Lattice("D3Q19")
    f_1 = orc.perturbed_init(SHAPE, lat, "FP32FP32", seed=7)
    pos, areas, vel = body()
    for tolerance, sweeps, expected in ((1e-5, 4, 4), (1.0, 4, 2), (0.0, 6, 6), (1.0, 1, 1)):
        assert emulation("D3Q19", "FP32FP32", f_1, pos, areas, vel, sweeps, tolerance)[2] == expected
    vel = vel * np.linspace(0.5, 1.5, len(pos), dtype=np.float32)[:, None]
    p = np.random.default_rng(5).permutation(len(pos))
    a = emulation("D3Q19", "FP32FP32", f_1, pos, areas, vel)
    b = emulation("D3Q19", "FP32FP32", f_1, pos[p], areas[p], vel[p])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][p], b[1])  # integer accumulation: bit-identical


def test_support_clipped_by_a_face_and_tiny_weight_sums(emulation):
    """Markers within two cells of the face z = 0 lose part of their support; cells at the very edge of a single support have weight
    sums down to 1e-10, where acc / W needs the per-cell quantum of the fixed-point sums."""
    lat = orc.Lattice("D3Q19")
    f_1 = orc.perturbed_init(SHAPE, lat, "FP64FP64", seed=7)
    pos, areas, vel = body(centre=(11.3, 12.6, 6.85))
    assert pos[:, 2].min() < 2.0
    exp = ref.couple(f_1, pos, areas, vel, lat, "FP64FP64", relaxation=0.5)
    f, F, used, cells = emulation("D3Q19", "FP64FP64", f_1, pos, areas, vel)
    W = exp["W"]
    assert 0 < W[W > 0].min() < 1e-8
    assert cells == int((W > 0).sum())
    assert np.abs(f - exp["f"]).max() <= 1e-9 and np.abs(F - exp["forces"]).max() <= 1e-9
