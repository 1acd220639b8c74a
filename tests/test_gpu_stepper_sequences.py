"""The sequences of tests/_stepper_sequences.py replayed on the device through the public API: every read is compared with the model bit
for bit, at the end every defined field and both masks, and the pairing counters (_n_fused_pairs, _n_materialised) of the stepper
objects with the restated lazy states.  One stepper (two for the ops that go through a second object) lives through a whole sequence:
whatever it caches — meta words, tile order, clean flags, the edge-kind scan, the scratch field, the fields' strips, a deferred step, a
virtual field — has to follow the ops (tests/test_stepper_sequences_cases.py checks without a GPU that the table can tell)."""

import numpy as np
import pytest

from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import HalfwayBounceBackBC
from xlb_amd.operator.equilibrium import QuadraticEquilibrium
from xlb_amd.operator.macroscopic import Macroscopic
from xlb_amd.operator.stepper import IncompressibleNavierStokesStepper
from xlb_amd.operator.stream import Stream
from xlb_amd.precision_policy import Precision

import _stepper_sequences as sq
from _util import init_hip, max_ulp_diff
from test_gpu_step2_matrix import assert_plan, hip_bc

pytestmark = pytest.mark.gpu


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape}, model {want.dtype} {want.shape}"
    if not np.array_equal(got, want):
        ulp = max_ulp_diff(got, want) if got.dtype.kind == "f" else "-"
        raise AssertionError(f"{what}: not bit-exact, {int((got != want).sum())} of {got.size} values differ, max ulp {ulp}")


class Device:
    """the device side of one grid of a sequence: what Grid is to the model"""

    def __init__(self, q, g, grid, fields):
        s = q.setup
        self.grid, self.halo = grid, s.halo
        self.cur, self.oth, self.bm, self.mm = fields
        vs_q = self.cur.cardinality
        self.t = 0
        self.new_pop = lambda: grid.create_field(vs_q, Precision.FP32)
        self.new_masks = lambda: (grid.create_field(1, Precision.UINT8), grid.create_missing_mask(vs_q))
        cp = Precision.FP64 if s.policy == "FP64FP32" else Precision.FP32
        self.rho, self.u = grid.create_field(1, cp), grid.create_field(3, cp)

    def upload_masks(self, v):
        self.bm.assign(v.bc_mask)
        self.mm.assign(v.missing_mask.astype(np.uint8))


def build(q):
    s = q.setup
    init_hip(s.lattice, s.policy)
    specs = sq.specs_of(s, 0, sq.variant_pos(s, 0, "rim"))
    bcs = [HalfwayBounceBackBC(profile=sq.plate, indices=sp.indices) if sp.params.get("profile") else hip_bc(sp) for sp in specs]
    assert [b.id for b in bcs] == [sp.id for sp in specs]
    cfg = {"halo": s.halo} if s.halo else None
    grids = [grid_factory(shape, backend_config=cfg) for shape in s.grids]
    steppers = [IncompressibleNavierStokesStepper(grid=grids[0], boundary_conditions=bcs, collision_type=s.collision) for _ in range(2)]
    devs = []
    for g, grid in enumerate(grids):
        rim = sq.setup_masks(s, g)[2]["rim"]
        if g == 0:
            fields = steppers[0].prepare_fields()  # the masker's masks: those of the oracle
            same_bits(fields[2].numpy(), rim.bc_mask, "the masker's bc_mask")
            same_bits(fields[3].numpy(), rim.missing_mask.astype(np.uint8), "the masker's missing_mask")
            d = Device(q, g, grid, fields)
        else:
            q19 = devs[0].cur.cardinality
            d = Device(q, g, grid, (grid.create_field(q19, Precision.FP32), grid.create_field(q19, Precision.FP32), grid.create_field(1, Precision.UINT8),
                                    grid.create_missing_mask(q19)))
            d.upload_masks(rim)
        d.cur.assign(sq.init_field(s, g, q.seed + g))
        d.oth.assign(np.zeros_like(sq.init_field(s, g, q.seed + g)))
        devs.append(d)
    return steppers, devs


def play(q, steppers, devs, ctx):
    s = q.setup
    sim = sq.Sim(s, q.seed)
    native = steppers[0]._native_stepper() if s.native else None
    lat = sq.setup_masks(s, 0)[0]
    if sq.time_dependent(s):
        assert steppers[0]._native_stepper().profile_slots() == sq.RING_SLOTS
    g = 0
    for i, op in enumerate(q.ops):
        kind, d = op[0], devs[g]
        what = f"op {i} {op}"
        exp = sim.apply(op)
        if kind in ("call", "call_noswap", "call_omega", "call_second", "call_gap"):
            d.t += kind == "call_gap"  # (a skipped timestep)
            stepper = steppers[1 if kind == "call_second" else 0]
            stepper(d.cur, d.oth, d.bm, d.mm, sq.OMEGAS[1] if kind == "call_omega" else sq.OMEGAS[0], d.t)
            if kind != "call_noswap":
                d.cur, d.oth = d.oth, d.cur
                d.t += 1
        elif kind == "run":
            a, b = d.cur, d.oth
            if native is not None:
                in_b = native.run(a, b, d.bm, d.mm, sq.OMEGAS[0], d.t, op[1])
                d.cur, d.oth = (b, a) if in_b else (a, b)
            else:
                d.cur, d.oth = steppers[0].run(a, b, d.bm, d.mm, sq.OMEGAS[0], op[1], first_timestep=d.t)
            assert (d.cur is b) == exp["result_in_b"], f"{what}: the result is in {'f_1' if d.cur is b else 'f_0'}"
            d.t += op[1]
        elif kind == "numpy":
            same_bits(getattr(d, op[1]).numpy(), exp["value"], what)
        elif kind == "get_plane":
            same_bits(getattr(d, op[1]).get_plane(op[2], op[3] + d.halo), exp["value"], what)
        elif kind == "macro":
            Macroscopic()(getattr(d, op[1]), d.rho, d.u)
            same_bits(d.rho.numpy(), exp["rho"], what + " rho")
            same_bits(d.u.numpy(), exp["u"], what + " u")
        elif kind == "sync":
            ctx.sync()
        elif kind == "mask_numpy":
            same_bits((d.bm if op[1] == "bm" else d.mm).numpy(), exp["value"], what)
        elif kind == "assign":
            getattr(d, op[1]).assign(sq.init_field(s, g, op[2]))
        elif kind == "set_plane":
            getattr(d, op[1]).set_plane(op[2], op[3] + d.halo, sq.init_field(s, g, op[4])[op[2], op[3]])
        elif kind == "fill":
            getattr(d, op[1]).fill(op[2])
        elif kind == "copy_from":
            d.oth.copy_from(d.cur)
        elif kind == "equilibrium":  # (rho, u) as orc.perturbed_init draws them: the operator's output is perturbed_init(seed)
            rng = np.random.default_rng(op[2])
            shape = s.grids[g]
            d.rho.assign((1.0 + 0.01 * rng.uniform(-1, 1, size=(1,) + shape)).astype(np.float32))
            d.u.assign((0.01 * rng.uniform(-1, 1, size=(lat.d,) + shape)).astype(np.float32))
            QuadraticEquilibrium()(d.rho, d.u, getattr(d, op[1]))
        elif kind == "stream":
            Stream()(d.cur, d.oth)
        elif kind == "touch":
            getattr(d, op[1]).touch()
        elif kind == "mask_assign":
            d.upload_masks(sq.setup_masks(s, g)[2][op[1]])
        elif kind == "mask_new":  # freed first: the new objects may get the old addresses
            d.bm.free()
            d.mm.free()
            d.bm, d.mm = d.new_masks()
            d.upload_masks(sq.setup_masks(s, g)[2][op[1]])
        elif kind == "fields_new":
            d.cur.free()
            d.oth.free()
            d.cur, d.oth = d.new_pop(), d.new_pop()
            d.cur.assign(sq.init_field(s, g, op[1]))
        elif kind == "pin":
            assert getattr(d, op[1]).__cuda_array_interface__["shape"] == getattr(d, op[1]).shape
        elif kind == "option":
            ctx.set_option(op[1], op[2])
        elif kind == "plan":
            assert_plan(steppers[0]._native_stepper().step2_plan(d.cur, d.oth, d.bm, d.mm), exp["plan"], what)
        elif kind == "grid":
            g = op[1]
        else:
            raise ValueError(kind)
    # the end: every defined field, both masks, the counters
    for g, (d, fin) in enumerate(zip(devs, sim.final())):
        for slot in ("cur", "oth"):
            if fin[slot] is not None:
                same_bits(getattr(d, slot).numpy(), fin[slot], f"final {slot} of grid {g}")
        v = sq.setup_masks(s, g)[2][fin["variant"]]
        same_bits(d.bm.numpy(), v.bc_mask, f"final bc_mask of grid {g}")
        same_bits(d.mm.numpy(), v.missing_mask.astype(np.uint8), f"final missing_mask of grid {g}")
    got = [(st._n_fused_pairs, st._n_materialised) for st in steppers]
    want = [(sim.n_fused[k], sim.n_materialised[k]) for k in (0, 1)]
    assert got == want, f"(fused pairs, materialisations) per stepper object: {got}, predicted {want}"


@pytest.mark.parametrize("q", sq.sequences(), ids=sq.seq_id)
def test_sequence(q):
    ctx = get_context()
    steppers = []
    try:
        for key, value in {**sq.OPTION_DEFAULTS, **dict(q.setup.base_options)}.items():
            ctx.set_option(key, value)
        steppers, devs = build(q)
        play(q, steppers, devs, ctx)
    finally:
        for st in steppers:  # a sequence that failed half way must not leave its deferred step to the next test's ctx.sync()
            st.abandon_deferred()
        for key, value in sq.OPTION_DEFAULTS.items():
            ctx.set_option(key, value)
