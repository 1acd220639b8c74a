"""The two-steps-per-pass kernel k_step2 (csrc/step2_kernel.hpp) across its work-item plan, against the oracle, bit for bit, and the
device's plan report (xlbhip_step2_plan) against the plan restated in tests/_step2_matrix.py: launches, ranges, tiles and every clean
flag.  The cases place one small boundary condition relative to the plan — next to tile seams, x-segment boundaries, thin end
segments, the box wrap — so that an item flagged clean that is not gives wrong bits here (tests/test_step2_matrix_cases.py checks
without a GPU that the table can tell)."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import EquilibriumBC, FullwayBounceBackBC, HalfwayBounceBackBC, RegularizedBC, ZouHeBC
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper

import _step2_matrix as m
from _util import init_hip, max_ulp_diff

pytestmark = pytest.mark.gpu

DEFAULTS = {"fuse2": 1, "fuse2_xseg": 0, "fuse2_clean": 1, "fuse2_strips": 1, "fuse2_rowmap": 0, "overlap": 1}


def hip_bc(spec):
    p = spec.params
    if spec.kind == orc.KIND_EQUILIBRIUM:
        return EquilibriumBC(rho=p["rho"], u=p["u"], indices=spec.indices)
    if spec.kind == orc.KIND_HALFWAY_BB:
        return HalfwayBounceBackBC(indices=spec.indices, prescribed_value=p.get("u_wall"))
    if spec.kind == orc.KIND_FULLWAY_BB:
        return FullwayBounceBackBC(indices=spec.indices)
    if spec.kind == orc.KIND_REGULARIZED_VELOCITY:
        return RegularizedBC("velocity", prescribed_value=p["prescribed"], indices=spec.indices)
    assert spec.kind == orc.KIND_ZOUHE_PRESSURE
    return ZouHeBC("pressure", prescribed_value=p["prescribed"], indices=spec.indices)


def set_options(ctx, setup, knobs, xseg=None):
    ctx.set_option("fuse2", 2)
    ctx.set_option("fuse2_xseg", setup.xseg if xseg is None else xseg)
    ctx.set_option("overlap", setup.overlap)
    ctx.set_option("fuse2_clean", knobs.clean)
    ctx.set_option("fuse2_strips", knobs.strips)
    ctx.set_option("fuse2_rowmap", knobs.rowmap)


def restore_options(ctx):
    for key, value in DEFAULTS.items():
        ctx.set_option(key, value)


def make_stepper(c):
    """a fresh stepper of the case with its fields; the masks are the masker's and equal the oracle's"""
    init_hip(c.setup.lattice)
    grid = grid_factory(c.setup.shape, backend_config={"halo": c.setup.halo} if c.setup.halo else None)
    specs = m.bc_specs(c.setup, c.background, c.probe, c.pos)
    bcs = [hip_bc(s) for s in specs]
    assert [b.id for b in bcs] == [s.id for s in specs]
    stepper = IncompressibleNavierStokesStepper(grid=grid, boundary_conditions=bcs)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    assert f_0.halo == c.setup.halo
    ms = m.case_masks(c)
    assert np.array_equal(bc_mask.numpy(), ms.bc_mask) and np.array_equal(missing_mask.numpy(), ms.missing_mask.astype(np.uint8)), "masks differ from the oracle's"
    return stepper, f_0, f_1, bc_mask, missing_mask


def assert_plan(report, restated, what):
    """the device's report of the next pass == the restated plan, field by field"""
    assert len(report) == len(restated), f"{what}: {len(report)} launches reported, {len(restated)} restated"
    for k, (got, (launch, flags)) in enumerate(zip(report, restated)):
        head = (got["x_begin"], got["x_count"], got["segments"], got["cap"], got["tile"], got["shift"], got["strips"], len(got["items"]))
        want = (launch.x_begin, launch.x_count, launch.segments, launch.cap, launch.tile, launch.shift, launch.strips, len(launch.items))
        assert head == want, f"{what}: launch {k} (x_begin, x_count, segments, cap, tile, shift, strips, items) = {head}, restated {want}"
        items = [tuple(int(v) for v in row[:3]) for row in got["items"]]
        assert items == list(launch.items), f"{what}: launch {k} items {items}, restated {list(launch.items)}"
        got_flags = [int(v) for v in got["items"][:, 3]]
        wrong = [(launch.items[i], got_flags[i], flags[i]) for i in range(len(flags)) if got_flags[i] != flags[i]]
        assert not wrong, f"{what}: launch {k} clean flags (item, device, restated) differ: {wrong}"


def assert_same_bits(out, exp, what):
    assert out.dtype == exp.dtype and out.shape == exp.shape
    assert np.array_equal(out, exp), f"{what}: not bit-exact, max ulp {max_ulp_diff(out, exp)}, {int((out != exp).sum())} of {out.size} values differ"


@pytest.mark.parametrize("c,knobs", [(c, k) for c in m.cases() for k in m.knob_sets(c)], ids=lambda v: m.case_id(v) if isinstance(v, m.Case) else v.name)
def test_step2_matrix_vs_plan_and_oracle(c, knobs):
    ctx = get_context()
    try:
        set_options(ctx, c.setup, knobs)
        stepper, f_0, f_1, bc_mask, missing_mask = make_stepper(c)
        native = stepper._native_stepper()
        assert native.step2_eligible(f_0, f_1, bc_mask, missing_mask)
        f_0.assign(m.f_init(c))
        assert_plan(native.step2_plan(f_0, f_1, bc_mask, missing_mask), m.restated_plan(c, knobs), "before the run")
        f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, c.omega, c.steps)
        # (across the knob sets of a case the bits are identical: each set gives the oracle's)
        assert_same_bits(f_0.numpy(), m.expected(c), knobs.name)
    finally:
        restore_options(ctx)


@pytest.mark.parametrize("c", [c for c in m.cases() if m.runs_reference_protocol(c)], ids=m.case_id)
def test_step2_matrix_reference_protocol(c):
    """stepper(f_0, f_1, ...) with the caller's swap: lazy pairing sends every two calls through xlbhip_step2 (fields without ghost
    planes; with them the calls stay single steps)"""
    ctx = get_context()
    try:
        set_options(ctx, c.setup, m.KNOBS[0])
        stepper, f_0, f_1, bc_mask, missing_mask = make_stepper(c)
        f_0.assign(m.f_init(c))
        for t in range(c.steps):
            f_0, f_1 = stepper(f_0, f_1, bc_mask, missing_mask, c.omega, t)
            f_0, f_1 = f_1, f_0
        assert_same_bits(f_0.numpy(), m.expected(c), "reference protocol")
        assert stepper._n_fused_pairs == (c.steps // 2 if c.setup.halo == 0 else 0)
    finally:
        restore_options(ctx)


def test_a_probe_moved_under_one_stepper():
    """The caches of ONE stepper (meta words, tile order, clean flags per launch geometry) follow the masks and the options: the probe
    moves rim position -> one further out -> another tile -> another segment by re-assigning bc_mask and missing_mask, and after each
    move fuse2_xseg goes 4 -> 3 -> 0 -> 4 and fuse2_clean 1 -> 0 -> 1; every run gives the oracle's bits and every plan report the
    restatement."""
    setup = m.SETUPS[0]
    assert setup.name == "x4" and setup.halo == 0
    sy, sz, starts = m.seams(setup, 1), m.seams(setup, 2), m.segment_starts(setup)
    inner = [m.interior_coord(setup, a) for a in range(3)]
    positions = [(inner[0], sy[0] - 1, inner[2]), (inner[0], sy[0] - 2, inner[2]), (inner[0], sy[1] + 2, sz[1] + 3), (starts[2] + 1, sy[1] + 2, sz[1] + 3)]
    base = m.Case(setup, "bare", "fw", positions[0], None, ("moved",), 4, 1.6, 4001, 0)
    ctx = get_context()
    try:
        set_options(ctx, setup, m.KNOBS[0])
        stepper, f_0, f_1, bc_mask, missing_mask = make_stepper(base)
        native = stepper._native_stepper()
        flags_seen = set()
        for k, pos in enumerate(positions):
            c = base._replace(pos=pos, seed=4001 + k, steps=m.STEPS[k % 4])
            ms = m.case_masks(c)
            bc_mask.assign(ms.bc_mask)
            missing_mask.assign(ms.missing_mask.astype(np.uint8))
            for xseg, clean in ((4, 1), (3, 0), (0, 1), (4, 1)):
                knobs = m.KNOBS[0] if clean else m.KNOBS[1]
                set_options(ctx, setup, knobs, xseg=xseg)
                what = f"probe at {pos}, fuse2_xseg={xseg}, fuse2_clean={clean}"
                assert native.step2_eligible(f_0, f_1, bc_mask, missing_mask), what
                f_0.assign(m.f_init(c))
                restated = m.restated_plan(c, knobs, xseg=xseg)
                assert_plan(native.step2_plan(f_0, f_1, bc_mask, missing_mask), restated, what)
                flags_seen.add((xseg, clean, tuple(restated[0][1])))
                f_0, f_1 = stepper.run(f_0, f_1, bc_mask, missing_mask, c.omega, c.steps)
                assert_same_bits(f_0.numpy(), m.expected(c), what)
        # the four positions give four different flag sets under (4, 1): a cache that kept the first would have been caught
        assert len({f for xseg, clean, f in flags_seen if (xseg, clean) == (4, 1)}) == 4
    finally:
        restore_options(ctx)
