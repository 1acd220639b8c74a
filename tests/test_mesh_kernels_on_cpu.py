"""The mesh voxelisers without a GPU: xlb_amd/csrc/masker_kernels.hpp is compiled for the host (tests/hip_on_cpu stands in for the HIP
runtime header, -ffp-contract=off as in the library's build), tests/mesh_cpu_emulation.cpp runs the kernels one emulated thread after
the other in the pass order of masker.hip, and bc_mask, missing_mask and the dense distances are compared with the oracle BIT FOR BIT,
on the cases tests/test_gpu_mesh_reference.py holds the GPU to (ORACLE_CASES of tests/_util.py, with and without distances).  This
checks the window rules, the overlap and segment tests, the link casts and the tagging rules — not the order in which the GPU's atomics
land nor its code generation.  The winding number sums fp64 atan2 values of the host's libm: a last-place difference from the device's
could only show at a voxel whose winding number is within rounding of 0.5, and no zoo mesh has one (profiles/mesh_reference.md)."""

import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import mesh_bc as mb
from oracle import xlb_numpy as orc

from _util import ORACLE_CASES, mesh_zoo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZOO = mesh_zoo()
LATTICE_ID = {"D3Q19": 1, "D3Q27": 2}
METHOD_ID = {"AABB": 1, "RAY": 2, "AABB_CLOSE": 3, "WINDING": 4}  # XLBHIP_MESH_*
ORACLE_ID = 3


@pytest.fixture(scope="module")
def emulation(tmp_path_factory):
    cxx = shutil.which("clang++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    if not cxx:
        pytest.skip("no clang++ to compile the kernel headers for the host")
    so = tmp_path_factory.mktemp("mesh_cpu") / "libmesh_cpu.so"
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", f"-I{os.path.join(ROOT, 'tests', 'hip_on_cpu')}",
                    f"-I{os.path.join(ROOT, 'xlb_amd', 'csrc')}", f"-I{os.path.join(ROOT, 'include')}", os.path.join(ROOT, "tests", "mesh_cpu_emulation.cpp"),
                    "-o", str(so)], check=True, timeout=600)
    lib = C.CDLL(str(so))
    lib.mesh_cpu.argtypes = [C.c_int] * 3 + [C.c_int64, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 3
    return lib


@functools.lru_cache(maxsize=None)
def oracle_masks(name, lattice, method, h):
    """as in tests/test_gpu_mesh_reference.py"""
    verts, shape = ZOO[name]
    lat = orc.Lattice(lattice)
    z1, zq, d0 = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool), np.zeros((lat.q,) + shape, np.float32)
    if method == "AABB":
        return orc.mesh_mask_aabb(shape, lat, ORACLE_ID, verts, z1, zq) + (None,)
    if method == "RAY":
        return mb.mesh_mask_ray(shape, lat, ORACLE_ID, verts, z1, zq, d0)
    if method == "WINDING":
        return mb.mesh_mask_winding(shape, lat, ORACLE_ID, verts, z1, zq, d0)
    return mb.mesh_mask_aabb_close(shape, lat, ORACLE_ID, verts, h, z1, zq, d0)


def run_emulated(lib, name, lattice, method, h, with_dist):
    """-> bc_mask (1, ...), missing_mask (q, ...) as bool, dense distances (q, ...) or None of one emulated masker call on fresh fields"""
    verts, shape = ZOO[name]
    q = orc.Lattice(lattice).q
    verts = np.ascontiguousarray(verts, np.float32)
    bc, bits = np.zeros((1,) + shape, np.uint8), np.zeros(shape, np.uint32)
    dist = np.zeros((q,) + shape, np.float32) if with_dist else None
    rc = lib.mesh_cpu(LATTICE_ID[lattice], METHOD_ID[method], ORACLE_ID, len(verts) // 3, verts.ctypes.data, h, *shape, bc.ctypes.data, bits.ctypes.data,
                      dist.ctypes.data if with_dist else None)
    assert rc == 0
    return bc, np.stack([(bits >> np.uint32(l)) & np.uint32(1) for l in range(q)]).astype(bool), dist


@pytest.mark.parametrize("name,lattice,method,h", ORACLE_CASES)
def test_emulated_kernels_vs_oracle_bit_for_bit(emulation, name, lattice, method, h):
    e_bc, e_mm, e_d = oracle_masks(name, lattice, method, h)
    for with_dist in (False, True) if method != "AABB" else (False,):
        got_bc, got_mm, got_d = run_emulated(emulation, name, lattice, method, h, with_dist)
        assert np.array_equal(got_bc, e_bc), f"bc_mask: {int((got_bc != e_bc).sum())} cells differ"
        assert np.array_equal(got_mm, e_mm), f"missing_mask: {int((got_mm != e_mm).sum())} bits differ"
        if with_dist:
            assert got_d.dtype == e_d.dtype == np.float32
            assert np.array_equal(got_d.view(np.uint32), e_d.view(np.uint32)), f"distances: {int((got_d.view(np.uint32) != e_d.view(np.uint32)).sum())} values differ"
