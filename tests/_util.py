"""Shared helpers for the parity tests: build the same case for the HIP backend
(xlb_amd, through the C ABI) and for the oracle, and compare."""

import os

import numpy as np

import xlb_amd
from oracle import xlb_numpy as orc
from xlb_amd import ComputeBackend, PrecisionPolicy
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import EquilibriumBC, FullwayBounceBackBC, HalfwayBounceBackBC
from xlb_amd.operator.macroscopic import Macroscopic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VS = {"D2Q9": xlb_amd.velocity_set.D2Q9, "D3Q19": xlb_amd.velocity_set.D3Q19, "D3Q27": xlb_amd.velocity_set.D3Q27}


def init_hip(lattice, policy="FP32FP32"):
    pp = PrecisionPolicy[policy]
    vs = VS[lattice](precision_policy=pp, compute_backend=ComputeBackend.HIP)
    xlb_amd.init(velocity_set=vs, default_backend=ComputeBackend.HIP, default_precision_policy=pp)
    return vs, pp


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def cavity_indices(grid, dim):
    """The index bookkeeping of the reference drivers (lid_driven_cavity_2d.py:43-49,
    mlups_3d.py:193-199)."""
    box = grid.bounding_box_indices()
    box_ne = grid.bounding_box_indices(remove_edges=True)
    lid = box_ne["top"]
    faces = ["bottom", "left", "right"] + (["front", "back"] if dim == 3 else [])
    walls = [sum((box[f][i] for f in faces), []) for i in range(dim)]
    walls = np.unique(np.array(walls), axis=-1).tolist()
    return lid, walls


def hip_cavity_2d(n, u_lid=0.05):
    """[walls, lid] with lid constructed first (lid_driven_cavity_2d.py:51-55)."""
    vs, pp = init_hip("D2Q9")
    grid = grid_factory((n, n))
    lid, walls = cavity_indices(grid, 2)
    bc_top = EquilibriumBC(rho=1.0, u=(u_lid, 0.0), indices=lid)
    bc_walls = HalfwayBounceBackBC(indices=walls)
    bcs = [bc_walls, bc_top]
    lat = orc.Lattice("D2Q9")
    obcs = [orc.BC(orc.KIND_HALFWAY_BB, bc_walls.id, walls), orc.BC(orc.KIND_EQUILIBRIUM, bc_top.id, lid, rho=1.0, u=(u_lid, 0.0))]
    return grid, bcs, lat, obcs


def hip_cavity_3d(shape, walls_cls, lattice="D3Q19", policy="FP32FP32", u_lid=0.02, backend_config=None):
    """[lid, walls] (mlups_3d.py:201-204)."""
    vs, pp = init_hip(lattice, policy)
    grid = grid_factory(shape, backend_config=backend_config)
    lid, walls = cavity_indices(grid, 3)
    bc_lid = EquilibriumBC(rho=1.0, u=(u_lid, 0.0, 0.0), indices=lid)
    bc_walls = walls_cls(indices=walls)
    kind = orc.KIND_FULLWAY_BB if walls_cls is FullwayBounceBackBC else orc.KIND_HALFWAY_BB
    lat = orc.Lattice(lattice)
    obcs = [orc.BC(orc.KIND_EQUILIBRIUM, bc_lid.id, lid, rho=1.0, u=(u_lid, 0.0, 0.0)), orc.BC(kind, bc_walls.id, walls)]
    return grid, [bc_lid, bc_walls], lat, obcs


def remap_ids(mask, mapping):
    out = mask.copy()
    for src, dst in mapping.items():
        out[mask == src] = dst
    return out


def hip_macroscopic(f, grid, vs, pp):
    macro = Macroscopic(velocity_set=vs, precision_policy=pp, compute_backend=ComputeBackend.HIP)
    rho = grid.create_field(1, dtype=pp.compute_precision)
    u = grid.create_field(vs.d, dtype=pp.compute_precision)
    macro(f, rho, u)
    return rho.numpy(), u.numpy()


def max_ulp_diff(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    it = {2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]
    ia, ib = a.view(it).astype(np.int64), b.view(it).astype(np.int64)
    sign = np.int64(1) << (8 * a.dtype.itemsize - 1)
    ia = np.where(ia < 0, -(ia + sign) - 0, ia)  # map sign-magnitude to a monotone integer line
    ib = np.where(ib < 0, -(ib + sign) - 0, ib)
    return int(np.abs(ia - ib).max())


def mesh_zoo():
    """{name: (vertices, grid shape)}: the procedural meshes of the mesh-voxeliser tests (tests/_mesh_ref.py holds the pieces).
    All but `integer_box` are in generic position: no vertex coordinate and no face plane on an integer or on k + 0.5, so that
    few links and voxels sit on a decision boundary.  The grids are multiples of no tile or block size."""
    import _mesh_ref as mr

    rot = mr.rotation()
    big, mid, small = (18, 16, 14), (17, 13, 11), (9, 10, 8)
    ctr = np.array([8.83, 7.87, 6.91])
    sphere = mr.rotated(icosphere(ctr, 4.23, 2), ctr, rot)  # 320 triangles: more than one 256-thread block
    generic = mr.rotated(mr.box((5.63, 4.71, 3.77), (11.91, 10.23, 9.39)), ctr, mr.rotation(angle=0.4))
    return {
        "sphere2": (sphere, big),
        "torus": (mr.torus(ctr, 4.63, 1.71, 24, 12, mr.rotation(angle=0.3)), big),  # 576 triangles, fluid cells in the hole
        "box": (generic, big),
        "box_low_faces": (mr.box((0.0, 0.0, 0.0), (5.37, 4.61, 3.29)), small),  # vertex coordinates 0.0 on the three low faces
        "box_high_faces": (mr.box((11.31, 7.43, 5.63), (16.995, 12.993, 10.991)), mid),  # ends within 0.01 of the high faces
        "plate": (mr.box((3.31, 2.43, 5.57), (13.63, 10.71, 5.87)), mid),  # 0.3 thick, between two planes of cell centres
        "two_boxes": (np.concatenate([mr.box((3.23, 4.31, 3.37), (7.62, 11.27, 9.71)), mr.box((8.32, 5.19, 4.13), (13.41, 10.63, 10.29))]), big),
        "sphere2_inward": (mr.inward(sphere), big),
        "box_zero_area": (mr.with_zero_area_triangle(generic), big),
        "integer_box": (mr.box((3.0, 4.0, 2.0), (7.0, 8.0, 6.0)), small),  # degenerate on purpose: never compared with the fp64 reference
    }


# the zoo meshes small enough for the oracle's per-triangle loops (12 - 24 triangles), and the cases (mesh, lattice, method,
# close_voxels) on which kernels and oracle must agree bit for bit: on the GPU and in the host-compiled emulation
ORACLE_MESHES = ["box", "box_low_faces", "box_high_faces", "plate", "two_boxes", "box_zero_area", "integer_box"]
ORACLE_CASES = [(name, "D3Q27", m, h) for name in ORACLE_MESHES for m, h in (("AABB", 0), ("RAY", 0), ("WINDING", 0), ("AABB_CLOSE", 2))]
ORACLE_CASES += [(name, "D3Q19", m, h) for name in ("box_low_faces", "integer_box") for m, h in (("AABB", 0), ("RAY", 0), ("WINDING", 0), ("AABB_CLOSE", 1))]


def icosphere(center, radius, subdivisions=2):
    """triangle soup (3 n, 3) of a sphere, counter-clockwise seen from outside, built procedurally (no STL reader here)"""
    t = (1.0 + 5.0**0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], float)
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6],
         [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    tris = v[np.array(f)]
    for _ in range(subdivisions):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = (a + b) / 2, (b + c) / 2, (c + a) / 2
        tris = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)])
    tris = tris / np.linalg.norm(tris, axis=2, keepdims=True)
    return (np.asarray(center) + radius * tris).reshape(-1, 3).astype(np.float32)
