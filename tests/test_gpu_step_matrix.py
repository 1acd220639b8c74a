"""The single-step kernel k_step<L, T, S, VEC, COLL, HASBC, FLAGS> (csrc/step_kernel.hpp) across its template matrix, against the
oracle, bit for bit: every lattice x collision x precision policy x cells per thread x boundary-condition variant that
step_launch.hpp instantiates (the cases of tests/_step_matrix.py, whose conditions tests/test_step_matrix_cases.py checks without a
GPU), the launch knobs (block shape, XCD swizzle, non-temporal accesses), and the fall-back from the two-step kernel."""

import itertools

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import (DoNothingBC, EquilibriumBC, ExtrapolationOutflowBC, FullwayBounceBackBC, HalfwayBounceBackBC,
                                                 RegularizedBC, ZouHeBC)
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

import _step_matrix as sm
from _util import hip_cavity_3d, init_hip, max_ulp_diff

pytestmark = pytest.mark.gpu


def hip_bc(spec):
    p = spec.params
    if spec.kind == orc.KIND_EQUILIBRIUM:
        return EquilibriumBC(rho=p["rho"], u=p["u"], indices=spec.indices)
    if spec.kind == orc.KIND_HALFWAY_BB:
        return HalfwayBounceBackBC(indices=spec.indices, prescribed_value=p.get("u_wall"))
    if spec.kind == orc.KIND_FULLWAY_BB:
        return FullwayBounceBackBC(indices=spec.indices)
    if spec.kind == orc.KIND_DO_NOTHING:
        return DoNothingBC(indices=spec.indices)
    if spec.kind == orc.KIND_EXTRAPOLATION_OUTFLOW:
        return ExtrapolationOutflowBC(indices=spec.indices)
    cls = RegularizedBC if spec.kind in (orc.KIND_REGULARIZED_VELOCITY, orc.KIND_REGULARIZED_PRESSURE) else ZouHeBC
    which = "velocity" if spec.kind in (orc.KIND_REGULARIZED_VELOCITY, orc.KIND_ZOUHE_VELOCITY) else "pressure"
    return cls(which, prescribed_value=p["prescribed"], indices=spec.indices)


def hip_bcs(c):
    """The case's boundary conditions, constructed in id order and listed in the case's order"""
    specs, order = sm.bc_specs(c)
    built = [hip_bc(s) for s in specs]
    assert [b.id for b in built] == [s.id for s in specs]
    return [built[i] for i in order]


def assert_same_bits(out, exp, what=""):
    assert out.dtype == exp.dtype
    assert np.array_equal(out, exp), f"{what}not bit-exact: max ulp {max_ulp_diff(out, exp)}, {int((out != exp).sum())} of {out.size} values differ"


@pytest.mark.parametrize("c", sm.cases(), ids=sm.case_id)
def test_step_matrix_vs_oracle(c, exact_math):
    init_hip(c.lattice, c.policy)
    ctx = get_context()
    coll, force = sm.collision_args(c)
    try:
        ctx.set_option("fuse2", 0)
        ctx.set_option("vec", c.vec)
        grid = grid_factory(c.shape)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=hip_bcs(c), collision_type=coll,
                                                    force_vector=None if force is None else np.array(force))
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        s = sm.setup(c)
        if c.bc_class != "none":
            assert np.array_equal(bc_mask.numpy(), s.bc_mask) and np.array_equal(missing_mask.numpy(), s.missing_mask.astype(np.uint8))
        f_0.assign(s.f_init)
        if c.refused:
            with pytest.raises(Exception, match=sm.EXT_REFUSAL):
                stepper.run(f_0, f_1, bc_mask, missing_mask, c.omega, c.steps)
            return
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, c.omega, c.steps)
        assert_same_bits(f_0.numpy(), sm.expected(c))
    finally:
        ctx.set_option("fuse2", 1)
        ctx.set_option("vec", 0)


# ---- launch knobs -------------------------------------------------------------------------------------------------------------------
KNOB_DEFAULTS = {"vec": 0, "block_tz": 0, "block_threads": 256, "xcd_swizzle": 0, "nt_load": 1, "nt_store": 1, "fuse2": 1}
KNOB_STEPS, KNOB_OMEGA = 3, 1.4

KNOB_FLOWS = [("D3Q19", "FP32FP32", "cavity"), ("D3Q27", "FP64FP32", "periodic"), ("D3Q19", "FP32FP16", "cavity")]


@pytest.mark.parametrize("shape,vec,block_tz", sm.KNOB_GEOMETRIES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
@pytest.mark.parametrize("lattice,policy,flow", KNOB_FLOWS)
def test_launch_knobs_do_not_change_the_result(lattice, policy, flow, shape, vec, block_tz):
    """block_tz, block_threads, xcd_swizzle, nt_load and nt_store change how the cells are dealt to threads and how memory is accessed,
    never what is computed: every combination gives the oracle's bits.  The geometries (tests/_step_matrix.py: KNOB_GEOMETRIES) make the
    swizzle live for either block size, with a partial last block row, and switch it off by itself in the others.  (A wrong blockIdx remap updates some cells twice and others
    not at all.)"""
    lat = orc.Lattice(lattice)
    if flow == "cavity":
        grid, bcs, lat, obcs = hip_cavity_3d(shape, HalfwayBounceBackBC, lattice=lattice, policy=policy)
        o_bm, o_mm = orc.build_masks(shape, lat, obcs)
    else:
        init_hip(lattice, policy)
        grid, bcs, obcs = grid_factory(shape), [], []
        o_bm, o_mm = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
    f_np = orc.perturbed_init(shape, lat, policy, seed=71, amp_rho=0.02, amp_u=0.03)
    exp = orc.run(f_np, o_bm, o_mm, obcs, KNOB_OMEGA, lat, KNOB_STEPS, policy)
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 0)
        ctx.set_option("vec", vec)
        ctx.set_option("block_tz", block_tz)
        stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        for swz, threads, ntl, nts in itertools.product((0, 1), (128, 256), (0, 1), (0, 1)):
            for key, value in (("xcd_swizzle", swz), ("block_threads", threads), ("nt_load", ntl), ("nt_store", nts)):
                ctx.set_option(key, value)
            f_0.assign(f_np)
            f_1.fill(0.0)
            if (lattice, nts, ntl) == ("D3Q19", 0, 1):
                # D3Q19 BGK is the one build with the tuning variants of the flags (step_d3q19_bgk.hip, launch_flags): it takes nt_store = 0
                # at its word, and non-temporal loads with plain stores are not among its variants — an error, not another kernel
                with pytest.raises(Exception, match="flag combination 2 not instantiated"):
                    stepper.run(f_0, f_1, bc_mask, missing_mask, KNOB_OMEGA, KNOB_STEPS)
                continue
            a, b = stepper.run(f_0, f_1, bc_mask, missing_mask, KNOB_OMEGA, KNOB_STEPS)
            assert_same_bits(a.numpy(), exp, f"xcd_swizzle={swz} block_threads={threads} nt_load={ntl} nt_store={nts}: ")
            f_0, f_1 = (a, b) if a is f_0 else (b, a)
    finally:
        for key, value in KNOB_DEFAULTS.items():
            ctx.set_option(key, value)


@pytest.mark.parametrize("vec", [1, 4])
def test_block_threads_above_the_launch_bound_is_refused(vec):
    init_hip("D3Q19")
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 0)
        ctx.set_option("vec", vec)
        ctx.set_option("block_threads", 512)
        stepper = IncompressibleNavierStokesStepper(grid=grid_factory((3, 8, 64)), boundary_conditions=[])
        f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
        with pytest.raises(Exception, match="exceeds the kernel's launch bound"):
            stepper.run(f_0, f_1, bc_mask, missing_mask, 1.0, 1)
    finally:
        for key, value in KNOB_DEFAULTS.items():
            ctx.set_option(key, value)


# ---- fall-back from the two-step kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["FP32FP16", "FP64FP64"])
@pytest.mark.parametrize("walls_cls", [None, HalfwayBounceBackBC])
def test_two_step_kernel_refuses_and_single_steps_take_over(policy, walls_cls):
    """fuse2 = 2 asks for the two-step kernel wherever it is eligible; it is built for 4-byte storage, so these policies are not, and an
    even-step run — all pairs, had it been — goes through k_step: the oracle's bits.  The same shape with FP32FP32 is eligible."""
    shape, omega, steps = (5, 8, 64), 1.6, 4
    ctx = get_context()
    try:
        ctx.set_option("fuse2", 2)
        for pol, eligible in (("FP32FP32", True), (policy, False)):
            if walls_cls is None:
                init_hip("D3Q19", pol)
                lat = orc.Lattice("D3Q19")
                grid, bcs, obcs = grid_factory(shape), [], []
                o_bm, o_mm = np.zeros((1,) + shape, np.uint8), np.zeros((lat.q,) + shape, bool)
            else:
                grid, bcs, lat, obcs = hip_cavity_3d(shape, walls_cls, policy=pol)
                o_bm, o_mm = orc.build_masks(shape, lat, obcs)
            stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
            f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
            assert bool(stepper._native_stepper().step2_eligible(f_0, f_1, bc_mask, missing_mask)) == eligible, pol
        f_np = orc.perturbed_init(shape, lat, policy, seed=73)
        f_0.assign(f_np)
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, omega, steps)
        assert_same_bits(f_0.numpy(), orc.run(f_np, o_bm, o_mm, obcs, omega, lat, steps, policy))
    finally:
        ctx.set_option("fuse2", 1)
