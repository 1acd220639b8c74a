"""MultiphaseStepper on the device against the NumPy restatement (tests/_multiphase_ref.py), bit for bit for the forms without a
transcendental (ShanChenDensity, CarnahanStarling): steps by __call__, the same by run, and the three output kernels, on the smallest
shapes at which the addressing can go wrong.  The exponential form's exp is ocml's, not NumPy's, so its chain is pinned piecewise: the
device's psi against an fp64 exp within PSI_EXP_MEASURED_ULPS + 1, and the populations bit for bit given the device's psi."""

import numpy as np
import pytest

from oracle import xlb_numpy as orc
from xlb_amd import _lib
from xlb_amd.default_config import get_context
from xlb_amd.grid import grid_factory
from xlb_amd.operator.boundary_condition import FullwayBounceBackBC, HalfwayBounceBackBC
from xlb_amd.operator.stepper import CarnahanStarling, MultiphaseStepper, ShanChenDensity, ShanChenExponential

import _multiphase_cases as cases
import _multiphase_ref as ref
from _util import init_hip, max_ulp_diff

pytestmark = pytest.mark.gpu

OMEGA = 1.2
T_CS = 0.8 * ref.CarnahanStarling.critical_temperature()
G_EXP = -5.5
# Largest difference, in ulps of the compute dtype, between the device's psi = rho0 (1 - exp(-rho / rho0)) and the same expression with
# np.exp evaluated in fp64 and rounded to the compute dtype, over 4096 densities in [0.01, 4] (rho0 = 1): measured on the first device run
# (profiles/multiphase.md; no accuracy table of the device's exp ships with the toolchain), plus one ulp for the rounding of the reference.
PSI_EXP_MEASURED_ULPS = {np.float32: 16, np.float64: 64}  # (4 and 4 above rho = 0.25: the figure is the cancellation's at the low end)

# (restatement model, device model, start state lo, hi, the two wall densities)
FORMS = {
    "density": (lambda: ref.Density(-0.6), lambda: ShanChenDensity(-0.6), 0.8, 1.2, 0.7, 1.1),
    "cs": (lambda: ref.CarnahanStarling(T_CS), lambda: CarnahanStarling(T_CS), 0.08, 0.3, 0.05, 0.25),
    "exp": (lambda: ref.Exponential(G_EXP), lambda: ShanChenExponential(G_EXP), 0.1, 2.5, 0.8, 1.8),
}

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


def assert_same_bits(out, exp, what=""):
    assert out.dtype == exp.dtype and out.shape == exp.shape, f"{what}: {out.dtype} {out.shape} against {exp.dtype} {exp.shape}"
    assert np.array_equal(out, exp), f"{what}: not bit-exact, max ulp {max_ulp_diff(out, exp)}, {int((out != exp).sum())} of {out.size} values differ"


class Device:
    """a set-up on the device and in the restatement's terms: the stepper, its fields with the set-up's masks, the oracle's BCs"""

    def __init__(self, build, lattice, policy, shape, form, force_vector=None):
        init_hip(lattice, policy)
        self.lat = orc.Lattice(lattice)
        self.policy, self.shape = policy, shape
        r_model, d_model, lo, hi, w_lo, w_hi = FORMS[form]
        self.model = r_model()
        setup = build(shape, w_lo, w_hi)
        d = self.lat.d
        bcs = []
        for w in setup.walls:
            if w.kind == orc.KIND_FULLWAY_BB:
                bcs.append(FullwayBounceBackBC(indices=w.indices))
            else:
                bcs.append(HalfwayBounceBackBC(indices=w.indices, prescribed_value=None if w.u_wall is None else list(w.u_wall)[:d]))
        self.obcs, self.wall_density = setup.oracle([bc.id for bc in bcs])
        by_id = {bc.id: bc for bc in bcs}
        wall_density = {("solid" if i == ref.BC_SOLID else by_id[i]): rho_w for i, rho_w in self.wall_density.items()}
        self.force_vector = force_vector
        self.stepper = MultiphaseStepper(grid_factory(shape), boundary_conditions=bcs, pseudopotential=d_model(), wall_density=wall_density,
                                         force_vector=force_vector)
        self.f_np = cases.random_state(shape, self.lat, policy, lo, hi, seed=29)
        self.f_0, self.f_1, self.bc_mask, self.missing_mask = self.stepper.prepare_fields(initializer=lambda bc_mask, f_0: f_0.assign(self.f_np))
        if bcs:  # the masker's masks are the oracle's; then the set-up's own corrections (solid cells, plates between periodic sides)
            raw_bm, raw_mm = orc.build_masks(shape, self.lat, self.obcs)
            assert np.array_equal(self.bc_mask.numpy(), raw_bm) and np.array_equal(self.missing_mask.numpy(), raw_mm.astype(np.uint8))
        self.bm, self.mm = setup.masks(shape, self.lat, self.obcs)
        if bcs:
            self.bc_mask.assign(self.bm)
            self.missing_mask.assign(self.mm.astype(np.uint8))

    def ref_kw(self):
        return dict(wall_density=self.wall_density, policy=self.policy, force_vector=self.force_vector)

    def ref_run(self, f, n):
        return ref.run(f, self.bm, self.mm, self.obcs, OMEGA, self.lat, self.model, n, **self.ref_kw())

    def ref_outputs(self, f, psi=None):
        return ref.outputs(f, self.bm, self.mm, self.obcs, self.lat, self.model, self.wall_density, self.policy, psi=psi)

    def restart(self):
        self.f_0.assign(self.f_np)
        self.f_1.fill(0.0)


# ---- the forms without a transcendental: everything bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["density", "cs"])
@pytest.mark.parametrize("name,build,lattice,policy,shape", CASES, ids=CASE_IDS)
def test_steps_and_outputs_match_the_restatement(name, build, lattice, policy, shape, form):
    dev = Device(build, lattice, policy, shape, form, force_vector=np.array([1e-4, -2e-4, 3e-4])[: 2 if lattice == "D2Q9" else 3])
    s, steps = dev.stepper, 3
    f_e = dev.ref_run(dev.f_np, steps)
    parts = dev.ref_outputs(f_e)
    assert np.isfinite(f_e).all() and np.isfinite(parts["psi"]).all() and np.abs(parts["force"]).max() > 1e-4
    f_0, f_1 = dev.f_0, dev.f_1
    for i in range(steps):
        f_0, f_1 = s(f_0, f_1, dev.bc_mask, dev.missing_mask, OMEGA, i)
        f_0, f_1 = f_1, f_0
    assert_same_bits(f_0.numpy(), f_e, "f by __call__")
    dev.restart()
    f, _ = s.run(dev.f_0, dev.f_1, dev.bc_mask, dev.missing_mask, OMEGA, steps)
    assert_same_bits(f.numpy(), f_e, "f by run")
    assert_same_bits(s.pseudopotential(f, dev.bc_mask, dev.missing_mask).numpy(), parts["psi"], "psi")
    assert_same_bits(s.interaction_force(f, dev.bc_mask, dev.missing_mask).numpy(), parts["force"], "force")
    rho, u = s.macroscopic(f, dev.bc_mask, dev.missing_mask)
    assert_same_bits(rho.numpy(), parts["rho"], "rho")
    assert_same_bits(u.numpy(), parts["u_phys"], "u")
    assert_same_bits(f.numpy(), f_e, "f after the output kernels")  # (they write nothing into the populations)


# ---- the exponential form: piecewise -----------------------------------------------------------------------------------------------------
def psi_exp_reference(rho, rho0=1.0):
    """rho0 (1 - exp(-rho / rho0)) in rho's dtype with exp evaluated in fp64 and rounded"""
    T = rho.dtype.type
    e = np.exp(-(rho / T(rho0)).astype(np.float64)).astype(T)
    return T(rho0) * (T(1) - e)


def psi_exp_bound(T):
    return PSI_EXP_MEASURED_ULPS[T] + 1


@pytest.mark.parametrize("policy", ["FP32FP32", "FP64FP64"])
def test_device_exp_over_a_density_sweep(policy):
    """4096 densities in [0.01, 4]: a ramp along the rows of a fluid at rest, which streaming leaves a ramp (one more cell at either end
    takes the wrap); the device's psi against the fp64 reference, in ulps of the compute dtype.  psi = 1 - e cancels at small densities:
    one ulp of e = exp(-0.01) is 64 ulps of psi, so the figure is that of the low end of the sweep."""
    lattice, n = "D2Q9", 4096
    shape = (3, n + 2)
    init_hip(lattice, policy)
    T = orc.compute_dtype(policy)
    lat = orc.Lattice(lattice)
    stepper = MultiphaseStepper(grid_factory(shape), pseudopotential=ShanChenExponential(G_EXP))
    h = (4.0 - 0.01) / (n - 1)
    ramp = np.linspace(0.01 - h, 4.0 + h, n + 2)
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields(density=np.broadcast_to(ramp, shape))
    bm, mm = ref.no_walls(shape, lat)
    _, rho, _ = ref.front(f_0.numpy(), bm, mm, [], lat, policy)
    rho = rho[0][:, 1:-1]
    assert abs(rho.min() - 0.01) < 1e-5 and abs(rho.max() - 4.0) < 1e-5
    psi = stepper.pseudopotential(f_0, bc_mask, missing_mask).numpy()[0][:, 1:-1]
    ulps = max_ulp_diff(psi, psi_exp_reference(rho))
    low = rho > 0.25
    print(f"{policy}: device psi against fp64 exp rounded to {T.__name__}: max {ulps} ulp over {rho.shape[1]} densities in [{rho.min():.4f}, {rho.max():.4f}]"
          f" ({max_ulp_diff(psi[low], psi_exp_reference(rho)[low])} ulp above 0.25)")
    assert ulps <= psi_exp_bound(T)


EXP_CASES = [CASES[0], CASES[1], CASES[6], CASES[7], CASES[9], CASES[10]]


@pytest.mark.parametrize("name,build,lattice,policy,shape", EXP_CASES, ids=[CASE_IDS[CASES.index(c)] for c in EXP_CASES])
def test_exponential_form_step_by_step_given_the_devices_psi(name, build, lattice, policy, shape):
    dev = Device(build, lattice, policy, shape, "exp")
    s = dev.stepper
    T = orc.compute_dtype(policy)
    f_0, f_1 = dev.f_0, dev.f_1
    f_np = dev.f_np
    for i in range(3):
        psi = s.pseudopotential(f_0, dev.bc_mask, dev.missing_mask).numpy()
        _, rho, _ = ref.front(f_np, dev.bm, dev.mm, dev.obcs, dev.lat, policy)
        table = ref.wall_table(dev.model, dev.wall_density, T)
        walls = ref.wall_cells(dev.bm, dev.obcs)
        expected = np.where(walls, table[dev.bm[0]], psi_exp_reference(rho[0]))[None]
        assert_same_bits(psi[0][walls], expected[0][walls], "psi at wall cells")
        ulps = max_ulp_diff(psi, expected)
        print(f"step {i}: psi within {ulps} ulp")
        assert ulps <= psi_exp_bound(T)
        parts = {}
        f_np = ref.step(f_np, dev.bm, dev.mm, dev.obcs, OMEGA, dev.lat, dev.model, psi=psi, parts=parts, **dev.ref_kw())
        assert np.isfinite(f_np).all() and np.abs(parts["force"]).max() > 1e-3
        assert_same_bits(s.interaction_force(f_0, dev.bc_mask, dev.missing_mask).numpy(), parts["force"], f"force, step {i}")
        f_0, f_1 = s(f_0, f_1, dev.bc_mask, dev.missing_mask, OMEGA, i)
        f_0, f_1 = f_1, f_0
        assert_same_bits(f_0.numpy(), f_np, f"f, step {i}")


# ---- the native loop -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 5])
def test_run_equals_n_calls_and_hands_back_the_result_first(n):
    dev = Device(cases.halfway_box, "D3Q19", "FP32FP32", (6, 6, 6), "exp")
    s = dev.stepper
    f_0, f_1 = dev.f_0, dev.f_1
    for i in range(n):
        f_0, f_1 = s(f_0, f_1, dev.bc_mask, dev.missing_mask, OMEGA, i)
        f_0, f_1 = f_1, f_0
    by_calls = f_0.numpy()
    dev.restart()
    f, f_other = s.run(dev.f_0, dev.f_1, dev.bc_mask, dev.missing_mask, OMEGA, n)
    assert (f is dev.f_1) == (n % 2 == 1) and f_other is not f
    assert_same_bits(f.numpy(), by_calls, "f")


def test_prepare_fields_sets_the_equilibrium_at_rest():
    init_hip("D3Q19", "FP32FP32")
    lat = orc.Lattice("D3Q19")
    shape = (4, 5, 6)
    stepper = MultiphaseStepper(grid_factory(shape), pseudopotential=ShanChenDensity(-0.5))
    rho = np.random.default_rng(2).uniform(0.5, 1.5, shape)
    assert_same_bits(stepper.prepare_fields(density=rho)[0].numpy(), ref.init_at_rest(rho, lat, "FP32FP32"), "f_0 from an array")
    assert_same_bits(stepper.prepare_fields(density=0.7)[0].numpy(), ref.init_at_rest(np.full(shape, 0.7), lat, "FP32FP32"), "f_0 from a number")
    with pytest.raises(ValueError, match="shape"):
        stepper.prepare_fields(density=np.ones((4, 5)))


def test_the_native_layer_refuses_what_the_kernels_cannot_take():
    init_hip("D3Q19", "FP32FP32")
    shape = (4, 4, 4)
    stepper = MultiphaseStepper(grid_factory(shape), pseudopotential=ShanChenDensity(-0.5))
    f_0, f_1, bc_mask, missing_mask = stepper.prepare_fields()
    before = f_1.numpy()
    for omega in (0.0, 2.5, float("nan")):
        with pytest.raises(Exception, match="outside"):
            stepper.run(f_0, f_1, bc_mask, missing_mask, omega, 2)
    with pytest.raises(Exception, match="different fields"):
        stepper.run(f_0, f_0, bc_mask, missing_mask, 1.0, 1)
    assert np.array_equal(f_1.numpy(), before)  # nothing was launched
    # below the Python refusal of fp16 storage: the kernels are built for three policies, and the create says so
    with pytest.raises(_lib.HipBackendError, match="built for FP32FP32, FP64FP64 and FP64FP32 only"):
        _lib.Multiphase(get_context(), _lib.D3Q19, _lib.F32, _lib.F16, [])


# ---- refusals at construction ----------------------------------------------------------------------------------------------------------
def test_refusals_at_construction():
    from xlb_amd.operator.boundary_condition import DoNothingBC, EquilibriumBC, ExtrapolationOutflowBC, HybridBC, RegularizedBC, ZouHeBC

    init_hip("D3Q19", "FP32FP32")
    shape = (8, 7, 8)
    grid = grid_factory(shape)
    f_ne = orc.bounding_box_indices(shape, remove_edges=True)
    model = ShanChenDensity(-0.5)
    for coll in ("KBC", "SmagorinskyLESBGK"):
        with pytest.raises(NotImplementedError, match=coll):
            MultiphaseStepper(grid, pseudopotential=model, collision_type=coll)
    with pytest.raises(ValueError, match="pseudopotential"):
        MultiphaseStepper(grid)
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
            MultiphaseStepper(grid, boundary_conditions=[make()], pseudopotential=model)
    with pytest.raises(NotImplementedError, match="profile"):
        MultiphaseStepper(grid, boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells: np.zeros_like(cells, dtype=float))],
                          pseudopotential=model)
    with pytest.raises(NotImplementedError, match="profile"):
        MultiphaseStepper(grid, boundary_conditions=[HalfwayBounceBackBC(indices=f_ne["bottom"], profile=lambda cells, timestep: np.zeros_like(cells, dtype=float))],
                          pseudopotential=model)
    mine, other = HalfwayBounceBackBC(indices=f_ne["bottom"]), HalfwayBounceBackBC(indices=f_ne["top"])
    with pytest.raises(ValueError, match="none of this stepper's"):
        MultiphaseStepper(grid, boundary_conditions=[mine], pseudopotential=model, wall_density={other: 1.0})
    with pytest.raises(ValueError, match="wall_density"):
        MultiphaseStepper(grid, boundary_conditions=[mine], pseudopotential=model, wall_density={mine: -1.0})
    with pytest.raises(NotImplementedError, match="slab"):
        MultiphaseStepper(grid_factory(shape, backend_config={"halo": 1}), pseudopotential=model)
    init_hip("D3Q19", "FP32FP16")
    with pytest.raises(NotImplementedError, match="fp16"):
        MultiphaseStepper(grid_factory(shape), pseudopotential=model)
