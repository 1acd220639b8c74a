"""The four mesh voxelisers of the HIP backend (k_mesh_* in csrc/masker_kernels.hpp) and the wall distances they hand to HybridBC
against the fp64 reference of tests/_mesh_ref.py, on a zoo of meshes chosen for what one easy sphere never runs: more triangles
than one 256-thread block (the tix >= n_tri guard, atomicMin / atomicOr between blocks), the clamps at the domain faces and tags
dropped outside the box, the padded grid of AABB_CLOSE next to a face, close_voxels 1 and 3, links that cross two surfaces (the
closest hit must win), an inward orientation and a zero-area triangle.  Every case runs the masker twice on fresh fields: the
results must not depend on the order in which the atomics land.

The reference is built once per mesh, over the cells within 3 of the mesh's bounding box; outside that window the kernels must
have written nothing.  Comparison, ambiguity caps and the distance tolerance are those of tests/test_mesh_reference.py."""

import functools

import numpy as np
import pytest

import _mesh_ref as mr
from oracle import mesh_bc as mb
from oracle import xlb_numpy as orc
from xlb_amd.helper import create_nse_fields
from xlb_amd.operator.boundary_condition import HybridBC
from xlb_amd.operator.boundary_masker import BC_SOLID, MeshVoxelizationMethod, mesh_masker_for

from _util import ORACLE_CASES, init_hip, mesh_zoo, remap_ids

pytestmark = pytest.mark.gpu

ZOO = mesh_zoo()
REFERENCE_MESHES = ["sphere2", "torus", "box", "box_low_faces", "box_high_faces", "plate", "two_boxes", "sphere2_inward", "box_zero_area"]
METHODS = [("AABB", 0, False), ("RAY", 0, False), ("RAY", 0, True), ("WINDING", 0, False), ("WINDING", 0, True), ("AABB_CLOSE", 2, False),
           ("AABB_CLOSE", 2, True)]
CASES = [(name, lattice) + m for name in REFERENCE_MESHES for lattice in ("D3Q19", "D3Q27") for m in METHODS]
CASES += [(name, lattice, "AABB_CLOSE", h, d) for name in ("box", "box_low_faces", "box_high_faces") for lattice in ("D3Q19", "D3Q27") for h in (1, 3)
          for d in (False, True)]
ORACLE_ID = 3


@functools.lru_cache(maxsize=None)
def reference(name):
    verts, shape = ZOO[name]
    return mr.MeshReference(verts, shape)


@functools.lru_cache(maxsize=None)
def oracle_masks(name, lattice, method, h):
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


def run_masker(name, lattice, method, h, with_dist):
    """-> (bc id, bc_mask (1, ...), missing_mask (q, ...), distance table or None) of one masker call on fresh fields"""
    init_hip(lattice)
    verts, shape = ZOO[name]
    grid, f_0, f_1, missing_mask, bc_mask = create_nse_fields(shape)
    vm = MeshVoxelizationMethod(method, close_voxels=h) if method == "AABB_CLOSE" else MeshVoxelizationMethod(method)
    bc = HybridBC("bounceback_regularized", mesh_vertices=verts.copy(), voxelization_method=vm, use_mesh_distance=with_dist)
    mesh_masker_for(bc.voxelization_method)(bc, f_1, bc_mask, missing_mask)
    return bc.id, bc_mask.numpy(), missing_mask.numpy(), bc._distance_table


def run_twice(name, lattice, method, h, with_dist):
    """The same call twice on fresh fields gives identical arrays, whatever the order of atomicMin / atomicOr between blocks"""
    a, b = run_masker(name, lattice, method, h, with_dist), run_masker(name, lattice, method, h, with_dist)
    assert np.array_equal(remap_ids(a[1], {a[0]: 1}), remap_ids(b[1], {b[0]: 1})) and np.array_equal(a[2], b[2])
    if with_dist:
        assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1].view(np.uint32), b[3][1].view(np.uint32))
    else:
        assert a[3] is None and b[3] is None
    return a


@pytest.mark.parametrize("name,lattice,method,h,with_dist", CASES)
def test_kernels_vs_reference(name, lattice, method, h, with_dist):
    ref = reference(name)
    bc_id, got_bc, got_mm, table = run_twice(name, lattice, method, h, with_dist)
    lat = orc.Lattice(lattice)
    req, amb, stats = ref.masks(method, lat.c, bc_id, h, with_dist)
    mr.check_caps(stats)
    got_d = None
    if with_dist:
        cells, w = table
        assert np.array_equal(cells, np.flatnonzero(got_bc.reshape(-1) == bc_id)) and w.shape == (len(cells), lat.q) and w.dtype == np.float32
        got_d = mr.dense_distances(table, lat.q, ref.shape)
    dis = mr.disagreements(req, amb, got_bc, got_mm, got_d)
    print(name, lattice, method, h, with_dist, stats, dis)
    assert dis["bc"] == 0 and dis["mm"] == 0 and dis["dist"] == 0, dis
    assert not got_bc[0][~ref.window].any() and not got_mm[:, ~ref.window].any()  # nothing written outside the window
    solid = got_bc[0] == BC_SOLID
    if method == "WINDING":
        if name in ("plate", "sphere2_inward"):
            assert not got_bc.any() and not got_mm.any()  # no centre inside / inward orientation: nothing solid, nothing tagged
        else:
            # watertight: a fluid voxel with a solid voxel at x - c_l carries the id and missing[l], except through ambiguous links
            links = 0
            for l in range(lat.q):
                c = tuple(int(x) for x in lat.c[:, l])
                if any(c):
                    through = ~solid & mr._shift(solid, tuple(-x for x in c)) & ~amb["mm"][l]
                    links += int(through.sum())
                    assert got_mm[l][through].all() and (got_bc[0][through] == bc_id).all()
            assert links > 200
    elif method == "RAY":
        assert not solid.any()
    elif method == "AABB":
        assert 0 < stats["solid_voxels"] <= solid.sum() <= stats["solid_voxels"] + stats["amb_voxels"]
    else:
        assert solid.any()


@pytest.mark.parametrize("name,lattice,method,h", ORACLE_CASES)
def test_kernels_vs_oracle_bit_for_bit(name, lattice, method, h):
    """Masks and weights equal the oracle's bit for bit on the small meshes, the box with every vertex on an integer included:
    it sits on every decision boundary there is, so only the oracle's fp32 operation order can say what the kernels must give."""
    e_bc, e_mm, e_d = oracle_masks(name, lattice, method, h)
    for with_dist in (False, True) if method != "AABB" else (False,):
        bc_id, got_bc, got_mm, table = run_twice(name, lattice, method, h, with_dist)
        assert np.array_equal(remap_ids(got_bc, {bc_id: ORACLE_ID}), e_bc) and np.array_equal(got_mm, e_mm.astype(np.uint8))
        if with_dist:
            cells, w = table
            exp_cells = np.flatnonzero(e_bc.reshape(-1) == ORACLE_ID)
            assert np.array_equal(cells, exp_cells)
            assert np.array_equal(w, e_d.reshape(e_d.shape[0], -1)[:, exp_cells].T)
