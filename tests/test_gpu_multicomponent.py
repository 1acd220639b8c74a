"""MulticomponentStepper on the device against the NumPy restatement (tests/_multicomponent_ref.py), bit for bit: steps by __call__, the
same by run with an odd and an even step count, and the output kernels (both densities, both forces, the physical velocity), on the
smallest shapes at which the row kernels' addressing can go wrong (those of tests/test_gpu_multiphase.py).  Unequal relaxation rates, a
force vector and three distinct non-zero interaction strengths (tests/_multicomponent_cases.py)."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd import _lib
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import FullwayBounceBackBC, HalfwayBounceBackBC
from xlb_amd.operator.stepper import MulticomponentStepper, ShanChenMixture

import _multicomponent_cases as cases
import _multicomponent_ref as ref
from _util import init_hip, max_ulp_diff

pytestmark = pytest.mark.gpu

OMEGA = cases.OMEGA

# (name, set-up, lattice, policy, shape)
CASES = [
    ("periodic", cases.periodic, "D3Q19", "FP32FP32", (5, 6, 7)),  # odd sizes wrap on every axis
    ("periodic", cases.periodic, "D3Q19", "FP64FP64", (5, 6, 7)),
    ("periodic", cases.periodic, "D3Q19", "FP64FP32", (5, 6, 7)),
    ("periodic", cases.periodic, "D3Q19", "FP32FP32", (2, 3, 4)),  # the two x neighbours are the same plane
    ("periodic", cases.periodic, "D3Q27", "FP32FP32", (4, 5, 6)),
    ("periodic", cases.periodic, "D2Q9", "FP64FP64", (7, 9)),
    ("long-walls", cases.long_walls, "D2Q9", "FP64FP64", (3, 320)),  # a row of two blocks, the second partly empty
    ("halfway-box", cases.halfway_box, "D3Q19", "FP32FP32", (6, 6, 6)),  # edge and corner cells with sideways missing bits
    ("halfway-box", cases.halfway_box, "D3Q19", "FP64FP32", (6, 6, 6)),
    ("fullway-box", cases.fullway_box, "D3Q19", "FP32FP32", (6, 6, 6)),
    ("solid-block", cases.solid_block, "D3Q19", "FP32FP32", (8, 8, 8)),
]
CASE_IDS = [f"{c[0]}-{c[2]}-{c[3]}-{'x'.join(map(str, c[4]))}" for c in CASES]


def mixture():
    return ShanChenMixture(G_AB=cases.G_AB, G_AA=cases.G_AA, G_BB=cases.G_BB)


def assert_same_bits(out, exp, what=""):
    assert out.dtype == exp.dtype and out.shape == exp.shape, f"{what}: {out.dtype} {out.shape} against {exp.dtype} {exp.shape}"
    assert np.array_equal(out, exp), f"{what}: not bit-exact, max ulp {max_ulp_diff(out, exp)}, {int((out != exp).sum())} of {out.size} values differ"


class Device:
    """a set-up on the device and in the restatement's terms: the stepper, its fields with the set-up's masks, the oracle's BCs"""

    def __init__(self, build, lattice, policy, shape):
        init_hip(lattice, policy)
        self.lat = orc.Lattice(lattice)
        self.policy, self.shape = policy, shape
        setup = build(shape, cases.WALL_LO, cases.WALL_HI)
        bcs = []
        for w in setup.walls:
            assert w.u_wall is None
            bcs.append(FullwayBounceBackBC(indices=w.indices) if w.kind == orc.KIND_FULLWAY_BB else HalfwayBounceBackBC(indices=w.indices))
        self.obcs, self.wall_density = setup.oracle([bc.id for bc in bcs])
        by_id = {bc.id: bc for bc in bcs}
        wall_density = {("solid" if i == ref.BC_SOLID else by_id[i]): pair for i, pair in self.wall_density.items()}
        self.force_vector = cases.force_vector(self.lat)
        self.stepper = MulticomponentStepper(grid_factory(shape), boundary_conditions=bcs, interaction=mixture(), wall_density=wall_density,
                                             force_vector=self.force_vector)
        self.fa_np, self.fb_np = cases.random_states(shape, self.lat, policy, seed=29)
        self.fa_0, self.fa_1, self.fb_0, self.fb_1, self.bc_mask, self.missing_mask = self.stepper.prepare_fields(
            initializer=lambda bc_mask, fa_0, fb_0: (fa_0.assign(self.fa_np), fb_0.assign(self.fb_np)))
        if bcs:  # the masker's masks are the oracle's; then the set-up's own corrections (solid cells, plates between periodic sides)
            raw_bm, raw_mm = orc.build_masks(shape, self.lat, self.obcs)
            assert np.array_equal(self.bc_mask.numpy(), raw_bm) and np.array_equal(self.missing_mask.numpy(), raw_mm.astype(np.uint8))
        self.bm, self.mm = setup.masks(shape, self.lat, self.obcs)
        if bcs:
            self.bc_mask.assign(self.bm)
            self.missing_mask.assign(self.mm.astype(np.uint8))
        self.masks = (self.bc_mask, self.missing_mask)

    def ref_run(self, n):
        return ref.run(self.fa_np, self.fb_np, self.bm, self.mm, self.obcs, OMEGA, self.lat, cases.mixture(), n, wall_density=self.wall_density,
                       policy=self.policy, force_vector=self.force_vector)

    def ref_outputs(self, fa, fb):
        return ref.outputs(fa, fb, self.bm, self.mm, self.obcs, self.lat, cases.mixture(), self.wall_density, self.policy)

    def restart(self):
        self.fa_0.assign(self.fa_np)
        self.fb_0.assign(self.fb_np)
        self.fa_1.fill(0.0)
        self.fb_1.fill(0.0)
        return self.fa_0, self.fa_1, self.fb_0, self.fb_1


@pytest.mark.parametrize("name,build,lattice,policy,shape", CASES, ids=CASE_IDS)
def test_steps_and_outputs_match_the_restatement(name, build, lattice, policy, shape):
    dev = Device(build, lattice, policy, shape)
    s = dev.stepper
    expected = {n: dev.ref_run(n) for n in (2, 3)}
    fa_e, fb_e = expected[3]
    parts = dev.ref_outputs(fa_e, fb_e)
    assert np.isfinite(fa_e).all() and np.isfinite(fb_e).all()
    assert min(np.abs(parts["force_a"]).max(), np.abs(parts["force_b"]).max()) > 1e-4
    fa_0, fa_1, fb_0, fb_1 = dev.fa_0, dev.fa_1, dev.fb_0, dev.fb_1
    for i in range(3):
        fa_0, fa_1, fb_0, fb_1 = s(fa_0, fa_1, fb_0, fb_1, *dev.masks, OMEGA, i)
        fa_0, fa_1, fb_0, fb_1 = fa_1, fa_0, fb_1, fb_0
    assert_same_bits(fa_0.numpy(), fa_e, "f_A by __call__")
    assert_same_bits(fb_0.numpy(), fb_e, "f_B by __call__")
    fa, fa_other, fb, fb_other = s.run(*dev.restart(), *dev.masks, OMEGA, 2)  # an even count: the result is back in the first fields
    assert fa is dev.fa_0 and fb is dev.fb_0 and fa_other is dev.fa_1 and fb_other is dev.fb_1
    assert_same_bits(fa.numpy(), expected[2][0], "f_A by run, 2 steps")
    assert_same_bits(fb.numpy(), expected[2][1], "f_B by run, 2 steps")
    fa, fa_other, fb, fb_other = s.run(*dev.restart(), *dev.masks, OMEGA, 3)  # an odd count
    assert fa is dev.fa_1 and fb is dev.fb_1 and fa_other is dev.fa_0 and fb_other is dev.fb_0
    assert_same_bits(fa.numpy(), fa_e, "f_A by run, 3 steps")
    assert_same_bits(fb.numpy(), fb_e, "f_B by run, 3 steps")
    psi_a, psi_b = s.densities(fa, fb, *dev.masks)
    assert_same_bits(psi_a.numpy(), parts["psi_a"], "rho_A as the force reads it")
    assert_same_bits(psi_b.numpy(), parts["psi_b"], "rho_B as the force reads it")
    force_a, force_b = s.interaction_force(fa, fb, *dev.masks)
    assert_same_bits(force_a.numpy(), parts["force_a"], "F_A")
    assert_same_bits(force_b.numpy(), parts["force_b"], "F_B")
    rho_a, rho_b, u = s.macroscopic(fa, fb, *dev.masks)
    assert_same_bits(rho_a.numpy(), parts["rho_a"], "rho_A")
    assert_same_bits(rho_b.numpy(), parts["rho_b"], "rho_B")
    assert_same_bits(u.numpy(), parts["u_phys"], "u")
    assert_same_bits(fa.numpy(), fa_e, "f_A after the output kernels")  # (they write nothing into the populations)
    assert_same_bits(fb.numpy(), fb_e, "f_B after the output kernels")


def test_a_single_omega_stands_for_both():
    dev = Device(cases.periodic, "D3Q19", "FP32FP32", (5, 6, 7))
    s = dev.stepper
    fa, _, fb, _ = s.run(*dev.restart(), *dev.masks, 1.1, 2)
    one_a, one_b = fa.numpy(), fb.numpy()
    fa, _, fb, _ = s.run(*dev.restart(), *dev.masks, (1.1, 1.1), 2)
    assert_same_bits(fa.numpy(), one_a, "f_A")
    assert_same_bits(fb.numpy(), one_b, "f_B")
    fa_e, fb_e = ref.run(dev.fa_np, dev.fb_np, dev.bm, dev.mm, dev.obcs, 1.1, dev.lat, cases.mixture(), 2, policy=dev.policy, force_vector=dev.force_vector)
    assert_same_bits(one_a, fa_e, "f_A against the restatement")
    assert_same_bits(one_b, fb_e, "f_B against the restatement")


def test_prepare_fields_from_numbers_and_from_arrays():
    init_hip("D3Q19", "FP32FP32")
    lat = orc.Lattice("D3Q19")
    shape = (4, 5, 6)
    stepper = MulticomponentStepper(grid_factory(shape), interaction=mixture())
    rng = np.random.default_rng(2)
    rho_a, rho_b = rng.uniform(0.5, 1.5, shape), rng.uniform(0.01, 0.4, shape)
    fields = stepper.prepare_fields(density=(rho_a, rho_b))
    assert len(fields) == 6
    assert_same_bits(fields[0].numpy(), ref.init_at_rest(rho_a, lat, "FP32FP32"), "f_A from an array")
    assert_same_bits(fields[2].numpy(), ref.init_at_rest(rho_b, lat, "FP32FP32"), "f_B from an array")
    fields = stepper.prepare_fields(density=(0.7, rho_b))
    assert_same_bits(fields[0].numpy(), ref.init_at_rest(np.full(shape, 0.7), lat, "FP32FP32"), "f_A from a number")
    assert_same_bits(fields[2].numpy(), ref.init_at_rest(rho_b, lat, "FP32FP32"), "f_B from an array beside a number")
    fields = stepper.prepare_fields(density=(0.7, 0.05))
    assert_same_bits(fields[2].numpy(), ref.init_at_rest(np.full(shape, 0.05), lat, "FP32FP32"), "f_B from a number")
    with pytest.raises(ValueError, match="shape"):
        stepper.prepare_fields(density=(np.ones((4, 5)), 1.0))
    with pytest.raises(ValueError, match="pair"):
        stepper.prepare_fields(density=1.0)
    # a non-positive density: the scheme divides by rho of either component
    for bad in ((0.0, 1.0), (1.0, -0.1), (np.where(rho_a > 1.0, 0.0, rho_a), 1.0), (1.0, -rho_b)):
        with pytest.raises(ValueError, match="positive"):
            stepper.prepare_fields(density=bad)


def test_the_native_layer_refuses_what_the_kernels_cannot_take():
    init_hip("D3Q19", "FP32FP32")
    shape = (4, 4, 4)
    stepper = MulticomponentStepper(grid_factory(shape), interaction=mixture())
    fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask = stepper.prepare_fields()
    before = fa_1.numpy()
    for omega in (0.0, (1.0, 2.5), (float("nan"), 1.0)):
        with pytest.raises(Exception, match="outside"):
            stepper.run(fa_0, fa_1, fb_0, fb_1, bc_mask, missing_mask, omega, 2)
    for fields in ((fa_0, fa_0, fb_0, fb_1), (fa_0, fa_1, fa_0, fb_1), (fa_0, fa_1, fb_0, fa_1)):
        with pytest.raises(Exception, match="different fields"):
            stepper.run(*fields, bc_mask, missing_mask, 1.0, 1)
    assert np.array_equal(fa_1.numpy(), before)  # nothing was launched
    # below the Python refusals: the kernels are built for three policies and for walls at rest, and the create says so
    with pytest.raises(_lib.HipBackendError, match="built for FP32FP32, FP64FP64 and FP64FP32 only"):
        _lib.Multicomponent(get_context(), _lib.D3Q19, _lib.F32, _lib.F16, [])
    moving = HalfwayBounceBackBC(indices=orc.bounding_box_indices(shape, remove_edges=True)["bottom"], prescribed_value=[0.01, 0.0, 0.0])
    with pytest.raises(_lib.HipBackendError, match="wall velocity"):
        _lib.Multicomponent(get_context(), _lib.D3Q19, _lib.F32, _lib.F32, [moving._hip_descriptor()])


def test_refusals_at_construction():
    from xlb_amd.operator.boundary_condition import DoNothingBC, EquilibriumBC, ExtrapolationOutflowBC, HybridBC, RegularizedBC, ZouHeBC

    init_hip("D3Q19", "FP32FP32")
    shape = (8, 7, 8)
    grid = grid_factory(shape)
    f_ne = orc.bounding_box_indices(shape, remove_edges=True)
    model = mixture()
    for coll in ("KBC", "SmagorinskyLESBGK", "RegularizedBGK"):
        with pytest.raises(NotImplementedError, match=coll):
            MulticomponentStepper(grid, interaction=model, collision_type=coll)
    with pytest.raises(ValueError, match="interaction"):
        MulticomponentStepper(grid)
    unsupported = [
        (lambda: EquilibriumBC(rho=1.0, u=(0.0, 0.0, 0.0), indices=f_ne["top"]), "EquilibriumBC"),
        (lambda: DoNothingBC(indices=f_ne["top"]), "DoNothingBC"),
        (lambda: ZouHeBC("velocity", prescribed_value=(0.01, 0.0, 0.0), indices=f_ne["left"]), "ZouHeBC"),
        (lambda: ZouHeBC("pressure", prescribed_value=1.0, indices=f_ne["right"]), "ZouHeBC"),
        (lambda: RegularizedBC("velocity", prescribed_value=(0.01, 0.0, 0.0), indices=f_ne["left"]), "RegularizedBC"),
        (lambda: ExtrapolationOutflowBC(indices=f_ne["right"]), "ExtrapolationOutflowBC"),
        (lambda: HybridBC("bounceback_regularized", indices=cases.block_cells(shape)), "HybridBC"),
    ]
    for make, name in unsupported:
        with pytest.raises(NotImplementedError, match=name):
            MulticomponentStepper(grid, boundary_conditions=[make()], interaction=model)
    with pytest.raises(NotImplementedError, match="profile"):
        MulticomponentStepper(grid, boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells: np.zeros_like(cells, dtype=float))],
                              interaction=model)
    with pytest.raises(NotImplementedError, match="profile"):
        MulticomponentStepper(grid, boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"],
                                                                             profile=lambda cells, timestep: np.zeros_like(cells, dtype=float))],
                              interaction=model)
    with pytest.raises(NotImplementedError, match="wall velocity"):
        MulticomponentStepper(grid, boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"], prescribed_value=[0.01, 0.0, 0.0])], interaction=model)
    mine, other = HalfwayBounceBackBC(indices=f_ne["bottom"]), HalfwayBounceBackBC(indices=f_ne["top"])
    with pytest.raises(ValueError, match="none of this stepper's"):
        MulticomponentStepper(grid, boundary_conditions=[mine], interaction=model, wall_density={other: (1.0, 0.1)})
    with pytest.raises(ValueError, match="wall_density"):
        MulticomponentStepper(grid, boundary_conditions=[mine], interaction=model, wall_density={mine: (-1.0, 0.1)})
    with pytest.raises(ValueError, match="pairs"):
        MulticomponentStepper(grid, boundary_conditions=[mine], interaction=model, wall_density={mine: 1.0})
    with pytest.raises(NotImplementedError, match="slab"):
        MulticomponentStepper(grid_factory(shape, backend_config={"halo": 1}), interaction=model)
    init_hip("D3Q19", "FP32FP16")
    with pytest.raises(NotImplementedError, match="fp16"):
        MulticomponentStepper(grid_factory(shape), interaction=model)
