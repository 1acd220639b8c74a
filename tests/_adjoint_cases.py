"""The boundary configurations the adjoint tests share (oracle descriptors), small enough for fp64 finite differences on the host."""

import numpy as np

from oracle import xlb_numpy as orc


def _union(*index_lists):
    return np.unique(np.concatenate([np.asarray(i) for i in index_lists], axis=1), axis=-1).tolist()


def periodic(lattice, shape):
    return orc.Lattice(lattice), tuple(shape), []


def cavity_halfway(lattice, shape):
    """lid = EquilibriumBC on the last axis' upper face without its edges, every other face a halfway wall"""
    return _cavity(lattice, shape, orc.KIND_HALFWAY_BB)


def cavity_fullway(lattice, shape):
    return _cavity(lattice, shape, orc.KIND_FULLWAY_BB)


def _cavity(lattice, shape, walls_kind):
    lat, shape = orc.Lattice(lattice), tuple(shape)
    box, box_ne = orc.bounding_box_indices(shape), orc.bounding_box_indices(shape, remove_edges=True)
    walls = _union(*[box[s] for s in box if s != "top"])
    u = (0.03,) + (0.0,) * (lat.d - 1)
    return lat, shape, [orc.BC(orc.KIND_EQUILIBRIUM, 1, box_ne["top"], rho=1.0, u=u), orc.BC(walls_kind, 2, walls)]


def moving_wall(lattice, shape):
    """a halfway wall with a wall velocity on top, a no-slip halfway wall at the bottom, periodic otherwise"""
    lat, shape = orc.Lattice(lattice), tuple(shape)
    box = orc.bounding_box_indices(shape)
    u = (0.03,) + (0.0,) * (lat.d - 1)
    return lat, shape, [orc.BC(orc.KIND_HALFWAY_BB, 1, box["top"], u_wall=u), orc.BC(orc.KIND_HALFWAY_BB, 2, box["bottom"])]


def do_nothing_channel(lattice, shape):
    """equilibrium inlet on the left, DoNothingBC on the right face (both without edges), fullway walls on every other face"""
    lat, shape = orc.Lattice(lattice), tuple(shape)
    box, box_ne = orc.bounding_box_indices(shape), orc.bounding_box_indices(shape, remove_edges=True)
    walls = _union(*[box[s] for s in box if s not in ("left", "right")])
    u = (0.02,) + (0.0,) * (lat.d - 1)
    return lat, shape, [orc.BC(orc.KIND_FULLWAY_BB, 1, walls), orc.BC(orc.KIND_EQUILIBRIUM, 2, box_ne["left"], rho=1.0, u=u),
                        orc.BC(orc.KIND_DO_NOTHING, 3, box_ne["right"])]


def masks(shape, lat, bcs):
    if bcs:
        return orc.build_masks(shape, lat, bcs)
    return np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)


# the host cases: the four of the prototype (cavity_2d(12), cavity_3d(6) fullway, cavity_3d(6) halfway D3Q27, a periodic D3Q19 box)
# plus a DoNothingBC outlet and a moving halfway wall
def _oracle_cavity_2d():
    return orc.cavity_2d(12)


def _oracle_cavity_3d_fullway():
    return orc.cavity_3d(6)


def _oracle_cavity_3d_halfway_q27():
    return orc.cavity_3d(6, orc.KIND_HALFWAY_BB, lattice="D3Q27")


HOST_CASES = {
    "cavity2d-halfway-D2Q9": _oracle_cavity_2d,
    "cavity3d-fullway-D3Q19": _oracle_cavity_3d_fullway,
    "cavity3d-halfway-D3Q27": _oracle_cavity_3d_halfway_q27,
    "periodic-D3Q19": lambda: periodic("D3Q19", (5, 4, 3)),
    "donothing-D2Q9": lambda: do_nothing_channel("D2Q9", (9, 8)),
    "movingwall-D3Q19": lambda: moving_wall("D3Q19", (5, 4, 6)),
}
