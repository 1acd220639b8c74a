"""The walled set-ups and start states shared by the multiphase tests (host emulation, device, physics pins): walls as plain
specifications, turned into oracle BCs once their ids are known, and a random state in a density range where every form stays real.
TEST INFRASTRUCTURE ONLY."""

import numpy as np

from oracle import xlb_numpy as orc

import _multiphase_ref as ref

U_WALL = {2: (0.02, 0.0), 3: (0.02, -0.01, 0.0)}  # tangential to the faces of the last axis


class Wall:
    """one boundary condition of a set-up: kind (oracle's), cells (d, n), a constant wall velocity or None, a wall density or None"""

    def __init__(self, kind, indices, rho_w=None, u_wall=None):
        self.kind, self.indices, self.rho_w, self.u_wall = kind, indices, rho_w, u_wall


class Setup:
    def __init__(self, walls, solid=None, solid_rho_w=None, plate_axis=None):
        self.walls, self.solid, self.solid_rho_w, self.plate_axis = walls, solid, solid_rho_w, plate_axis

    def oracle(self, ids=None):
        """(oracle BCs, {bc id: wall density}) with the ids given (default 1, 2, ...)"""
        ids = list(range(1, len(self.walls) + 1)) if ids is None else list(ids)
        bcs = [orc.BC(w.kind, i, w.indices, u_wall=w.u_wall) for w, i in zip(self.walls, ids)]
        wall_density = {i: w.rho_w for w, i in zip(self.walls, ids) if w.rho_w is not None}
        if self.solid_rho_w is not None:
            wall_density[ref.BC_SOLID] = self.solid_rho_w
        return bcs, wall_density

    def masks(self, shape, lat, bcs):
        """The masker's masks, the solid cells retagged 255 (what a mesh masker leaves behind).  Plates between periodic sides: only the
        directions that come out of a plate are missing (the masker also flags those that leave the box sideways at the plates' edge
        cells, which would put a piece of side wall there and break the conservation of mass)."""
        bm, mm = orc.build_masks(shape, lat, bcs) if bcs else ref.no_walls(shape, lat)
        if self.plate_axis is not None:
            a = self.plate_axis % lat.d
            face = [slice(None)] * (lat.d + 1)
            for at, sign in ((0, 1), (-1, -1)):
                face[a + 1] = at
                mm[tuple(face)] = (lat.c[a] == sign).reshape((lat.q,) + (1,) * (lat.d - 1))
        if self.solid is not None:
            bm[(0,) + tuple(np.asarray(self.solid))] = ref.BC_SOLID
        return bm, mm


def random_state(shape, lat, policy, lo, hi, seed, amp_u=0.02):
    """f = feq(rho, u), rho ~ U(lo, hi), u ~ U(-amp_u, amp_u), in the store dtype"""
    T = orc.compute_dtype(policy)
    rng = np.random.default_rng(seed)
    rho = rng.uniform(lo, hi, size=(1,) + tuple(shape)).astype(T)
    u = (amp_u * rng.uniform(-1, 1, size=(lat.d,) + tuple(shape))).astype(T)
    return orc.equilibrium(rho, u, lat, T).astype(orc.store_dtype(policy))


def box_faces(shape, axis=-1):
    """cell indices (d, n) of a closed box: the low face of `axis`, its high face, every other boundary cell"""
    grid = np.indices(shape).reshape(len(shape), -1)
    on_edge = np.any((grid == 0) | (grid == np.array(shape)[:, None] - 1), axis=0)
    low, high = grid[axis] == 0, grid[axis] == shape[axis] - 1
    return grid[:, low].tolist(), grid[:, high].tolist(), grid[:, on_edge & ~low & ~high].tolist()


def block_cells(shape):
    """a 2 x 3 x 2 block in the interior of a 3-D box"""
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    inside = (abs(x - shape[0] // 2 + 0.5) < 1.1) & (abs(y - shape[1] // 2) < 1.6) & (abs(z - shape[2] // 2 + 0.5) < 1.1)
    return [a.tolist() for a in np.nonzero(inside)]


def periodic(shape, rho_lo, rho_hi):
    return Setup([])


def halfway_box(shape, rho_lo, rho_hi):
    """closed by halfway walls: two wall densities on the two faces of the last axis (the side walls: none), the high face moving"""
    low, high, sides = box_faces(shape)
    H = orc.KIND_HALFWAY_BB
    return Setup([Wall(H, low, rho_lo), Wall(H, high, rho_hi, u_wall=U_WALL[len(shape)]), Wall(H, sides)])


def fullway_box(shape, rho_lo, rho_hi):
    low, high, sides = box_faces(shape)
    F = orc.KIND_FULLWAY_BB
    return Setup([Wall(F, low, rho_lo), Wall(F, high, rho_hi), Wall(F, sides, rho_lo)])


def halfway_plates(shape, rho_lo, rho_hi, axis=-1):
    """halfway walls on the two faces of `axis`; the other axes stay periodic"""
    low, high, _ = box_faces(shape, axis)
    return Setup([Wall(orc.KIND_HALFWAY_BB, low, rho_lo), Wall(orc.KIND_HALFWAY_BB, high, rho_hi)], plate_axis=axis)


def long_walls(shape, rho_lo, rho_hi):
    """halfway walls on the faces of the FIRST axis (the long faces of a 3 x 320 strip)"""
    return halfway_plates(shape, rho_lo, rho_hi, axis=0)


def solid_block(shape, rho_lo, rho_hi):
    """an index-built block in a periodic box: its cells get id 255, the fluid cells around it keep the halfway BC's id and missing bits"""
    cells = block_cells(shape)
    return Setup([Wall(orc.KIND_HALFWAY_BB, cells, rho_lo)], solid=cells, solid_rho_w=rho_hi)
