"""The face arms of the two-step kernel's boundary waves (step2_kernel.hpp, bc_arm): a wave whose union of missing bits lies inside
the c_z = +1 set (wall at z = 0) or the c_z = -1 set (wall at z = nz - 1) sends only those 5 of 19 populations through the
halfway-wall redirect machinery and treats the other 14 as a fluid wave does; every other union takes the generic arm.  The arms
must not change a bit: D3Q19 BGK FP32FP32 pairs of steps (fuse2 = 2) on a 24 x 16 x 128 box — two tile rows and two tile columns of
the half-tile-shifted (8 x 64) tiling, so the wrap-around tile row and column and one interior tile all exist — from a perturbed
state, 2 ... 5 steps (odd and even counts, the write-only strip pass and the passes that read strips), all 19 populations compared
with np.array_equal against oracle/xlb_numpy.py."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import FullwayBounceBackBC, HalfwayBounceBackBC
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

from _util import hip_cavity_3d, init_hip, max_ulp_diff

pytestmark = pytest.mark.gpu

SHAPE = (24, 16, 128)
OMEGA = 1.6
STEPS = (2, 3, 4, 5)
U_WALL = (0.01, 0.005, 0.0)
# a solid 4 x 4 x 4 block given by interior indices; the tiling is shifted by (4, 32) cells, so tile boundaries lie at
# y = 12 and z = 32: the block straddles both
BLOCK = [a.ravel().tolist() for a in np.meshgrid(np.arange(10, 14), np.arange(10, 14), np.arange(30, 34), indexing="ij")]


def _scenario(name):
    """-> grid, HIP boundary conditions, oracle boundary conditions"""
    if name == "cavity_halfway":  # the bench's cavity: z-face row waves with the c_z = +1 union, edge and corner rows with mixed ones
        grid, bcs, _, obcs = hip_cavity_3d(SHAPE, HalfwayBounceBackBC)
        return grid, bcs, obcs
    if name == "cavity_fullway":
        grid, bcs, _, obcs = hip_cavity_3d(SHAPE, FullwayBounceBackBC)
        return grid, bcs, obcs
    init_hip("D3Q19")
    grid = grid_factory(SHAPE)
    box = grid.bounding_box_indices()
    if name == "periodic":
        return grid, [], []
    if name == "six_walls":  # no lid: the lanes z = nz - 1 miss the c_z = -1 set, a row wave holds both signs -> generic arm
        walls = np.unique(np.array([sum((box[f][i] for f in ("bottom", "top", "left", "right", "front", "back")), []) for i in range(3)]), axis=-1).tolist()
        bc = HalfwayBounceBackBC(indices=walls)
        return grid, [bc], [orc.BC(orc.KIND_HALFWAY_BB, bc.id, walls)]
    if name == "top_wall":  # a wall on z = nz - 1 alone, periodic elsewhere: the pure c_z = -1 union
        bc = HalfwayBounceBackBC(indices=box["top"])
        return grid, [bc], [orc.BC(orc.KIND_HALFWAY_BB, bc.id, box["top"])]
    if name == "moving_bottom_wall":  # a moving wall on z = 0 alone: the moving-wall term inside the c_z = +1 arm
        bc = HalfwayBounceBackBC(indices=box["bottom"], prescribed_value=U_WALL)
        return grid, [bc], [orc.BC(orc.KIND_HALFWAY_BB, bc.id, box["bottom"], u_wall=U_WALL)]
    if name == "solid_block":  # interior solid: unions with c_x, c_y and both c_z signs -> generic arm
        bc = HalfwayBounceBackBC(indices=BLOCK)
        return grid, [bc], [orc.BC(orc.KIND_HALFWAY_BB, bc.id, BLOCK)]
    raise ValueError(name)


_expected = {}  # scenario -> {steps: f}: the oracle runs once per scenario


def _oracle(name, obcs):
    if name not in _expected:
        lat = orc.Lattice("D3Q19")
        if obcs:
            o_bm, o_mm = orc.build_masks(SHAPE, lat, obcs)
        else:
            o_bm, o_mm = np.zeros((1,) + SHAPE, np.uint8), np.zeros((lat.q,) + SHAPE, bool)
        f = orc.perturbed_init(SHAPE, lat, seed=57)
        states = {0: f}
        for s in range(1, max(STEPS) + 1):
            f = orc.step(f, o_bm, o_mm, obcs, OMEGA, lat)
            states[s] = f
        for v in states.values():
            v.setflags(write=False)
        _expected[name] = states
    return _expected[name]


def _run_hip(grid, bcs, f_init, steps, fuse2, strips):
    ctx = get_context()
    try:
        ctx.set_option("fuse2", fuse2)
        ctx.set_option("fuse2_strips", strips)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        if fuse2 == 2:
            assert stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)
        f_0.assign(f_init)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, OMEGA, steps)
        return f_0.numpy()
    finally:
        ctx.set_option("fuse2", 1)
        ctx.set_option("fuse2_strips", 1)


def _check(name, steps, strips=1, single_steps_too=False):
    grid, bcs, obcs = _scenario(name)
    states = _oracle(name, obcs)
    out = _run_hip(grid, bcs, states[0], steps, 2, strips)
    exp = states[steps]
    assert out.shape == exp.shape == (19,) + SHAPE and out.dtype == exp.dtype
    assert np.array_equal(out, exp), f"max ulp {max_ulp_diff(out, exp)}, max abs {np.abs(out - exp).max()}"
    if single_steps_too:
        grid, bcs, _ = _scenario(name)  # a stepper of its own, with boundary-condition objects of its own
        single = _run_hip(grid, bcs, states[0], steps, 0, strips)
        assert np.array_equal(single, out), f"max ulp {max_ulp_diff(single, out)}"


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("strips", [0, 1])
def test_cavity_z_face_waves_take_the_cz_plus_arm(strips, steps):
    """The bench's cavity (lid = EquilibriumBC on the top face, halfway walls elsewhere), with and without strip buffers: its z-face
    row waves hold one wall lane, z = 0 (c_z = +1 arm); its edge and corner rows and its y- and x-face waves fall through to the
    generic arm.  Pairs and single steps give the same array."""
    _check("cavity_halfway", steps, strips=strips, single_steps_too=True)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("name", ["six_walls", "top_wall"])
def test_cz_minus_unions(name, steps):
    """Halfway walls on all six faces (a row wave of the z-face tile column holds z = 0 AND z = nz - 1: the union c_z = +1 | c_z = -1
    takes the generic arm), and a wall on z = nz - 1 alone in a periodic box (the pure c_z = -1 arm)."""
    _check(name, steps)


@pytest.mark.parametrize("steps", STEPS)
def test_moving_wall_inside_a_face_arm(steps):
    """A halfway wall with a non-zero wall velocity on z = 0 only: the moving-wall kind inside the c_z = +1 arm."""
    _check("moving_bottom_wall", steps)


@pytest.mark.parametrize("steps", STEPS)
def test_interior_solid_falls_through_to_the_generic_arm(steps):
    """A solid 4 x 4 x 4 halfway block given by interior indices, straddling a tile boundary in y and in z.  Pairs and single steps
    give the same array."""
    _check("solid_block", steps, single_steps_too=True)


@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("name", ["cavity_fullway", "periodic"])
def test_other_paths_are_untouched(name, steps):
    """Fullway cavity (no halfway lane: the fluid arm of the BC kernel) and periodic box (the BC-free kernel)."""
    _check(name, steps)
